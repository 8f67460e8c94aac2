"""tests/golden/py360_cube.npz from the REFERENCE'S OWN external/py360convert (numpy + scipy, runs in the build
container): e2c and c2e on three small shapes each (odd sizes, odd face widths), uint8 RGB and float32 with two
channels, bilinear and nearest, with the reference's own float32 sampling coordinates and, per shape, eps_meas = the
largest distance between those coordinates and the same formulas in float64 (tests/py360_cube_model.py).  The caps of
DESIGN.md 4.2 are asserted here on the reference alone, before anything is written.

    python tools/make_golden_py360_cube.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import py360_cube_model as M  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402

ORDER = {"bilinear": 1, "nearest": 0}


def pano_inputs(rng, H, W):
    return {"u8": (rng.random((H, W, 3)) * 255).astype(np.uint8), "f32": rng.standard_normal((H, W, 2)).astype(np.float32)}


def cube_inputs(rng, F):
    """Every face its own level and spread, so that a wrong neighbour, flip or pad row shows."""
    level = np.repeat(np.array([20, 60, 100, 140, 180, 215]), F)[None, :, None]
    u8 = (level + rng.random((F, 6 * F, 3)) * 40).astype(np.uint8)
    f32 = (rng.standard_normal((F, 6 * F, 2)) + (level - 120) / 40.0).astype(np.float32)
    return {"u8": u8, "f32": f32}


def main():
    sys.path.insert(0, REFERENCE_ROOT)
    ref = importlib.import_module("external.py360convert")
    ru = importlib.import_module("external.py360convert.utils")
    rng = np.random.default_rng(11)
    out = dict(e2c_shapes=np.array(M.E2C_SHAPES), c2e_shapes=np.array(M.C2E_SHAPES), eps_factor=M.EPS_FACTOR)
    report = []

    for i, (H, W, F) in enumerate(M.E2C_SHAPES):
        coor = ru.uv2coor(ru.xyz2uv(ru.xyzcube(F)), H, W)                      # e2c.py:20-22, float32
        assert coor.dtype == np.float32
        mx, my = M.e2c_coords(H, W, F)
        eps_meas = float(max(np.abs(coor[..., 0] - mx).max(), np.abs(coor[..., 1] - my).max()))
        out["e2c_%d_coor" % i], out["e2c_%d_eps_meas" % i], out["e2c_%d_eps" % i] = coor, eps_meas, M.EPS_FACTOR * eps_meas
        for key, img in pano_inputs(rng, H, W).items():
            out["e2c_%d_%s_in" % (i, key)] = img
            for mode, order in ORDER.items():
                want = ref.e2c(img, F, mode, "horizon")
                out["e2c_%d_%s_%s" % (i, key, mode)] = want
                share = M.check(M.e2c(img, F, order), want, M.e2c_setup(img, F), order, M.EPS_FACTOR * eps_meas,
                                "e2c %s %s %s" % ((H, W, F), key, mode))
                report.append(("e2c", (H, W, F), key, mode, eps_meas, share))
                if i == 1:
                    out["e2c_%d_%s_%s_dice" % (i, key, mode)] = ref.e2c(img, F, mode, "dice")

    seen = {}
    inner = ru.sample_cubefaces

    def recording(cube_faces, tp, coor_y, coor_x, order):
        seen.update(tp=tp, coor_y=coor_y, coor_x=coor_x)
        return inner(cube_faces, tp, coor_y, coor_x, order)

    ru.sample_cubefaces = recording
    try:
        for i, (h, w, F) in enumerate(M.C2E_SHAPES):
            for key, cube in cube_inputs(rng, F).items():
                out["c2e_%d_%s_in" % (i, key)] = cube
                for mode, order in ORDER.items():
                    want = ref.c2e(cube, h, w, mode, "horizon")
                    assert want.dtype == np.float64
                    out["c2e_%d_%s_%s" % (i, key, mode)] = want
                    # the coordinates are float32 values scaled in float64, (c + 0.5) * F exactly: stored as float32
                    c32 = np.stack([seen["coor_x"] / F - 0.5, seen["coor_y"] / F - 0.5], -1).astype(np.float32)
                    assert np.array_equal((c32[..., 0].astype(np.float64) + 0.5) * F, seen["coor_x"])
                    assert np.array_equal((c32[..., 1].astype(np.float64) + 0.5) * F, seen["coor_y"])
                    tp, mx, my = M.c2e_coords(h, w, F)
                    assert np.array_equal(tp, seen["tp"])
                    eps_meas = float(max(np.abs(seen["coor_x"] - mx).max(), np.abs(seen["coor_y"] - my).max()))
                    out["c2e_%d_coor" % i], out["c2e_%d_tp" % i] = c32, tp.astype(np.int8)
                    out["c2e_%d_eps_meas" % i], out["c2e_%d_eps" % i] = eps_meas, M.EPS_FACTOR * eps_meas
                    share = M.check(M.c2e(cube, h, w, order), want, M.c2e_setup(cube, h, w), order,
                                    M.EPS_FACTOR * eps_meas, "c2e %s %s %s" % ((h, w, F), key, mode))
                    report.append(("c2e", (h, w, F), key, mode, eps_meas, share))
                    if i == 1:
                        dice = ru.cube_h2dice(cube)
                        assert np.array_equal(ref.c2e(dice, h, w, mode, "dice"), want)
                        out["c2e_%d_%s_in_dice" % (i, key)] = dice
    finally:
        ru.sample_cubefaces = inner

    for path, shape, key, mode, eps_meas, share in report:
        print("%s %-12s %-3s %-8s eps_meas %.3e  excused / two-valued %.2f %%" % (path, shape, key, mode, eps_meas, 100 * share))
    p = os.path.join(ROOT, "tests", "golden", "py360_cube.npz")
    np.savez_compressed(p, **out)
    print(p, os.path.getsize(p) // 1024, "KiB")
    assert os.path.getsize(p) < 800 * 1024


if __name__ == "__main__":
    main()
