"""Device time of the cube-map kernels at the sizes their users run, next to the time the same
bytes take at the HBM rate: c2e of six 1024^2 uint8 RGB faces to 1024 x 2048 (the Matterport3D stitching shape), float64
and uint8 outputs; e2c of a 512 x 1024 uint8 RGB panorama to face_w 256.  Tensors stay on the GPU (no copies timed).
    python tools/py360_cube_bench.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from panfusion_amd.external.py360convert import c2e_batch, e2c_batch  # noqa: E402

DEV = "cuda"
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12          # bytes / s: specification, and what a float4 copy reaches


def timed(fn, window_s=0.5):
    """us per call from device events over a window of about ``window_s`` (three such windows: min and max)."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(10, int(window_s * 1e3 / max(e0.elapsed_time(e1) / 10, 1e-3)))
    out = []
    for _ in range(3):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return min(out), max(out), reps


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator().manual_seed(0)
    cube = torch.randint(0, 256, (1, 1024, 6144, 3), generator=g, dtype=torch.uint8).to(DEV)
    pano = torch.randint(0, 256, (1, 512, 1024, 3), generator=g, dtype=torch.uint8).to(DEV)
    rows = [
        ("c2e 6 x 1024^2 u8 RGB -> 1024 x 2048 float64", lambda: c2e_batch(cube, 1024, 2048), cube.numel() + 1024 * 2048 * 3 * 8),
        ("c2e 6 x 1024^2 u8 RGB -> 1024 x 2048 uint8", lambda: c2e_batch(cube, 1024, 2048, out_dtype=np.uint8),
         cube.numel() + 1024 * 2048 * 3),
        ("c2e the same, nearest, uint8", lambda: c2e_batch(cube, 1024, 2048, mode="nearest", out_dtype=np.uint8),
         cube.numel() + 1024 * 2048 * 3),
        ("e2c 512 x 1024 u8 RGB -> face_w 256", lambda: e2c_batch(pano, 256), pano.numel() + 6 * 256 * 256 * 3),
    ]
    for name, fn, byt in rows:
        lo, hi, reps = timed(fn)
        print("%-48s %8.1f .. %8.1f us (%d calls per window)   %6.2f MB: %5.1f us at 8.0 TB/s, %5.1f us at 6.3 TB/s"
              % (name, lo, hi, reps, byt / 1e6, byt / HBM_SPEC * 1e6, byt / HBM_COPY * 1e6))


if __name__ == "__main__":
    main()
