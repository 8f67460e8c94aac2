"""Geometry fixtures beyond the benchmark cameras, from the REFERENCE'S OWN e2p / p2e / get_masks / get_coords
(same recipe as tools/make_golden_grids.py): tests/golden/geometry_cameras.npz

One camera list (`camera_list`, repeated in tests/test_gpu_geometry.py, which checks that the two agree): 24 seeded
random cameras -- any field of view in [35, 130], yaw in [-400, 760] (outside one turn, fractional), any pitch -- and
ten edge cameras (poles, the +-180 seam, 360 = 0, a yaw that is no divisor of 360, very wide and very narrow views).
34 cameras cross the 12-camera launch batches of pf_geometry.hip at 12/13 and at 24/25.

What is recorded (digests are `digest` of tests/test_oracle_vs_reference.py: SHA-256 of the float64 / int64 values):
  * e2p grids (e2p.py:39-51) at E2P_SIZES and p2e grids + visibility masks (p2e.py:9-49) at P2E_SIZES: one digest per
    camera and size, the masks bit-packed, the full float64 maps at the smallest (odd, non-square) size only;
  * e2p / p2e tensor outputs (e2p.py:54-76, p2e.py:52-71), nearest and bilinear, of a seeded 3-channel image, one
    sample per camera, 32x64 <-> 12x20: digests;
  * get_masks (models/pano/utils.py:10-84) for the five-camera set CAMS5 at MASK_SHAPES and for the first 13 cameras
    of the list at (4,4 | 4,8): digests and the float32 arrays (the GPU table test compares with them);
  * get_coords (utils.py:87-106) for the list at (12,20 | 16,32): digest and arrays.

The file is written with fixed zip timestamps, so that a second run reproduces it byte for byte.

    python tools/make_golden_geometry.py        (build container only: imports the reference tree)
"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "geometry_cameras.npz")
MAX_BYTES = 735 * 1000                         # the largest fixture part committed so far

EDGE_CAMERAS = ((90, 0, 0), (90, 0, 90), (90, 0, -90), (90, 180, 0), (90, 360, 0),
                (90, -180, 45), (120, 359.999, 89.9), (60, 360 / 7, 0), (150, 12.5, -30), (20, 270, 10))
CAMS5 = np.array([[90, 70, 110, 90, 60], [0, 33.3, 200, -45, 123.4], [0, 90, -60, 20, -89]], dtype=np.float64).T
E2P_SIZES = ((16, 32, 16, 16), (32, 64, 12, 20), (17, 33, 9, 7), (64, 128, 32, 32))        # (eh, ew, h, w)
P2E_SIZES = ((16, 16, 16, 32), (12, 20, 32, 64), (9, 7, 17, 33))                           # (ph, pw, H, W)
MASK_SHAPES = ((8, 8, 8, 16), (6, 10, 8, 16), (4, 4, 4, 8))                                # (ph, pw, eh, ew)
REMAP_CASE = (32, 64, 12, 20)                                                              # panorama <-> view
COORD_SHAPE = (12, 20, 16, 32)


def camera_list():
    """(34, 3) float64 rows (FoV, theta, phi) in degrees: 24 seeded random cameras, then the ten edge cameras."""
    rng = np.random.default_rng(7)
    fov = np.round(rng.uniform(35, 130, 24), 3)                  # three draws of 24, in this order
    theta = np.round(rng.uniform(-400, 760, 24), 3)
    phi = np.round(rng.uniform(-90, 90, 24), 3)
    return np.concatenate([np.stack([fov, theta, phi], axis=1), np.array(EDGE_CAMERAS, dtype=np.float64)])


def remap_images():
    """The seeded panorama / view batch of the remap case: (34, 3, 32, 64) and (34, 3, 12, 20) float32."""
    rng = np.random.default_rng(8)
    eh, ew, h, w = REMAP_CASE
    return (torch.from_numpy(rng.standard_normal((34, 3, eh, ew)).astype(np.float32)),
            torch.from_numpy(rng.standard_normal((34, 3, h, w)).astype(np.float32)))


def camera_dict(cams):
    return {"FoV": torch.tensor(cams[:, 0]), "theta": torch.tensor(cams[:, 1]), "phi": torch.tensor(cams[:, 2])}


def digest(*arrays):
    """SHA-256 of the VALUES of a sequence of arrays (copy of tests/test_oracle_vs_reference.py:digest)."""
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.dtype.kind == "f":
            a = a.astype(np.float64) + 0.0
        elif a.dtype.kind in "iu":
            a = a.astype(np.int64)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def size_key(size):
    return "%dx%d_%dx%d" % size


def save_reproducibly(path, arrays):
    """np.savez_compressed with the zip members' timestamps fixed (numpy stamps them with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref = ref_import.load()
    cams = camera_list()
    out = dict(cams=cams, cams5=CAMS5)

    for size in E2P_SIZES:
        eh, ew, h, w = size
        maps = [ref.map_pers_pix_to_equi(eh, ew, f, t, p, h, w) for f, t, p in cams]
        out["e2p_grid_" + size_key(size)] = np.stack([digest(*m) for m in maps])
        if size == (17, 33, 9, 7):
            out["e2p_maps_" + size_key(size)] = np.stack([np.stack(m) for m in maps])            # (34, 2, h, w) float64
    for size in P2E_SIZES:
        ph, pw, H, W = size
        maps = [ref.map_equi_pix_to_pers(ph, pw, f, t, p, H, W) for f, t, p in cams]
        out["p2e_grid_" + size_key(size)] = np.stack([digest(*m) for m in maps])
        out["p2e_mask_" + size_key(size)] = np.packbits(np.stack([m[2] for m in maps]))
        if size == (9, 7, 17, 33):
            out["p2e_maps_" + size_key(size)] = np.stack([np.stack(m[:2]) for m in maps])        # (34, 2, H, W) float64

    pano, views = remap_images()
    eh, ew, h, w = REMAP_CASE
    cl = [torch.tensor(cams[:, k]) for k in range(3)]
    for mode in ("nearest", "bilinear"):
        out["remap_e2p_" + mode] = digest(ref.e2p(pano, *cl, (h, w), mode=mode))
        out["remap_p2e_" + mode] = digest(*ref.p2e(views, *cl, (eh, ew), mode=mode))

    sets = [("cams5_" + size_key(s), CAMS5, s) for s in MASK_SHAPES] + [("first13_" + size_key(MASK_SHAPES[2]), cams[:13], MASK_SHAPES[2])]
    for name, c, shape in sets:
        pers, equi = ref.get_masks(*shape, camera_dict(c), "cpu")
        out["masks_%s_digest" % name] = digest(pers, equi)
        out["masks_%s_pers" % name], out["masks_%s_equi" % name] = pers.numpy(), equi.numpy()

    pers, equi = ref.get_coords(*COORD_SHAPE, camera_dict(cams), "cpu")
    out["coords_digest"], out["coords_pers"], out["coords_equi"] = digest(pers, equi), pers.numpy(), equi.numpy()

    save_reproducibly(OUT, out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
