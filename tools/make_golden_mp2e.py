"""tests/golden/mp2e.npz from the REFERENCE'S OWN tensor p2e (external/Perspective_and_Equirectangular/p2e.py:52-71,
imported through oracle.ref_import; runs in the build container only): for every case of tests/mp2e_model.py the seeded
views and cameras and, per mode and feather,

    out   float64 (B, C, H, W): sum_i p2e(img_i) p2e(tent_i) / sum_i p2e(tent_i) on float64 views, 255 where the sum is 0
    wsum  float64 (B, H, W):    sum_i p2e(tent_i)
    e32, e32_w: the largest absolute difference between the same composition run in float32 (views, tent and sums) and
                out / wsum -- what the reference's own float32 path loses, the unit of the GPU tests' bounds.

The float32 and float64 runs must agree on the set wsum == 0 exactly, and tests/mp2e_model.py must reproduce out to float64
rounding; both are asserted here before anything is written.

    python tools/make_golden_mp2e.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mp2e_model as M  # noqa: E402
from oracle import ref_import  # noqa: E402


def cameras(ref, name, rng):
    """(B, m) degrees: FoV, theta, phi."""
    if name == "ico":
        theta, phi = ref.icosahedron_sample_camera()
        return np.full((1, 20), 90.0), np.rad2deg(theta)[None], np.rad2deg(phi)[None]
    if name == "hor":                                           # batch 1: the same ring turned and tilted
        theta, phi = ref.horizon_sample_camera(8)
        theta, phi = np.rad2deg(theta), np.rad2deg(phi)
        return np.full((2, 8), 90.0), np.stack([theta, theta + 17.0]), np.stack([phi, phi + 25.0])
    if name == "rnd":
        return rng.uniform(40, 110, (1, 5)), rng.uniform(-180, 180, (1, 5)), rng.uniform(-60, 60, (1, 5))
    if name == "one":
        return np.array([[75.0]]), np.array([[30.0]]), np.array([[20.0]])
    if name == "w2":
        return np.array([[90.0, 70.0]]), np.array([[0.0, 50.0]]), np.array([[0.0, -15.0]])
    raise KeyError(name)


def stitch(p2e, imgs, fov, theta, phi, out_hw, mode, feather, dtype):
    """One batch entry, everything (views, tent, products, sums) in ``dtype``."""
    m, C, h, w = imgs.shape
    views = torch.from_numpy(imgs).to(dtype)
    tent = torch.from_numpy(M.tent_image(h, w, feather, np.float64 if dtype == torch.float64 else np.float32))[None, None]
    assert tent.dtype == dtype
    num = torch.zeros(C, *out_hw, dtype=dtype)
    den = torch.zeros(*out_hw, dtype=dtype)
    for i in range(m):
        cam = (float(fov[i]), float(theta[i]), float(phi[i]))
        img, _ = p2e(views[i:i + 1], *cam, out_hw, mode)
        wgt, _ = p2e(tent, *cam, out_hw, mode)
        num += img[0] * wgt[0, 0]
        den += wgt[0, 0]
    zero = den == 0
    out = torch.where(zero, torch.tensor(255.0, dtype=dtype), num / torch.where(zero, torch.ones((), dtype=dtype), den))
    return out.numpy(), den.numpy()


def main():
    ref = ref_import.load()
    rng = np.random.default_rng(23)
    store = {}
    for name, spec in M.CASES.items():
        (h, w), out_hw, C, B = spec["view"], spec["pano"], spec["C"], spec["B"]
        fov, theta, phi = cameras(ref, name, rng)
        imgs = rng.uniform(0, 255, (B, fov.shape[1], C, h, w))
        store.update({name + "_imgs": imgs.astype(np.float32), name + "_fov": fov, name + "_theta": theta, name + "_phi": phi})
        imgs = imgs.astype(np.float32).astype(np.float64)        # the float64 run sees the values the float32 views hold
        for mode in M.MODES:
            for feather in spec["feathers"]:
                r64 = [stitch(ref.p2e, imgs[b], fov[b], theta[b], phi[b], out_hw, mode, feather, torch.float64) for b in range(B)]
                r32 = [stitch(ref.p2e, imgs[b], fov[b], theta[b], phi[b], out_hw, mode, feather, torch.float32) for b in range(B)]
                out64, w64 = (np.stack(a) for a in zip(*r64))
                out32, w32 = (np.stack(a) for a in zip(*r32))
                assert out64.dtype == w64.dtype == np.float64 and out32.dtype == w32.dtype == np.float32
                assert np.array_equal(w64 == 0, w32 == 0), (name, mode, feather, int(((w64 == 0) != (w32 == 0)).sum()))
                model = [M.mp2e(imgs[b], fov[b], theta[b], phi[b], out_hw, mode, feather) for b in range(B)]
                m_out, m_w = (np.stack(a) for a in zip(*model))
                assert np.array_equal(m_w == 0, w64 == 0) and np.abs(m_out - out64).max() <= 1e-9, (name, mode, feather)
                e32, e32_w = float(np.abs(out32 - out64).max()), float(np.abs(w32 - w64).max())
                k = M.key(name, mode, feather)
                store.update({k + "_out": out64, k + "_wsum": w64, k + "_e32": e32, k + "_e32_w": e32_w})
                pos = w64[w64 > 0]
                print("%-22s e32 %.2e  e32_w %.2e  uncovered %5.1f %%  smallest positive weight %.2e  model %.1e"
                      % (k, e32, e32_w, 100 * float((w64 == 0).mean()), float(pos.min()), float(np.abs(m_out - out64).max())))
    p = os.path.join(ROOT, "tests", "golden", "mp2e.npz")
    np.savez_compressed(p, **store)
    print(p, os.path.getsize(p) // 1024, "KiB")
    assert os.path.getsize(p) < 400 * 1024


if __name__ == "__main__":
    main()
