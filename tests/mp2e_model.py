"""Float64 numpy statement of mp2e (multi-perspective -> equirectangular stitch) on the tensor p2e semantics, shared by
tests/test_mp2e_cpu.py, tests/test_gpu_mp2e.py and tools/make_golden_mp2e.py (which pins it to the reference's own p2e):

    out = sum_i p2e(img_i) p2e(tent_i) / sum_i p2e(tent_i),   fill where the denominator is 0

p2e = grid_sample(align_corners=True, zeros outside) at the positions of oracle.geometry.p2e_grid, times the visibility
mask.  Not a test module (no test_ prefix)."""
import numpy as np

from oracle import geometry as G

MODES = ("bilinear", "nearest")

# name -> view (h, w), panorama (H, W), channels, batch, feathers.  Cameras and images are the fixture's (seeded there).
CASES = {
    "ico": dict(view=(16, 16), pano=(32, 64), C=3, B=1, feathers=("horizontal", "both")),   # 20 cameras > one by-value batch of 12
    "hor": dict(view=(8, 8), pano=(16, 32), C=3, B=2, feathers=("horizontal",)),            # half the sphere uncovered: fill
    "rnd": dict(view=(12, 20), pano=(24, 48), C=5, B=1, feathers=("horizontal", "both")),   # non-square, per-view FoV, small weights
    "one": dict(view=(10, 14), pano=(20, 40), C=1, B=1, feathers=("horizontal",)),          # m = 1
    "w2": dict(view=(4, 2), pano=(8, 16), C=3, B=1, feathers=("horizontal",)),              # linspace(num=1)
}


def keys():
    """(case, mode, feather) of every fixture entry."""
    return [(c, mode, f) for c, spec in CASES.items() for mode in MODES for f in spec["feathers"]]


def key(case, mode, feather):
    return "%s_%s_%s" % (case, mode, feather)


def tent(n):
    """The feather weights over n (even) columns, float64: linspace(0, 1, n/2) then linspace(1, 0, n/2)."""
    if n % 2:
        raise ValueError("the tent needs an even size, got %d" % n)
    return np.concatenate([np.linspace(0, 1, n // 2), np.linspace(1, 0, n // 2)])


def tent_image(h, w, feather, dtype=np.float64):
    """(h, w) weight image in ``dtype``: the tents are rounded to dtype first, their product (feather both) formed in dtype."""
    tx = tent(w).astype(dtype)
    if feather == "both":
        return tent(h).astype(dtype)[:, None] * tx[None, :]
    if feather != "horizontal":
        raise ValueError(feather)
    return np.broadcast_to(tx[None, :], (h, w)).copy()


def position(coord, size):
    """kornia's normalisation (factor first) and grid_sample's un-normalisation (align_corners=True), float64."""
    factor = 2.0 / (size - 1)
    xn = factor * coord - 1.0
    return ((xn + 1.0) / 2.0) * (size - 1)


def sample(img, u, v, mode):
    """img (C, h, w), pixel maps u, v (H, W) -> (C, H, W) float64, zeros outside."""
    img = np.asarray(img, np.float64)
    _, h, w = img.shape
    px, py = position(u, w), position(v, h)

    def tap(ix, iy):
        ok = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
        return np.where(ok[None], img[:, np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)], 0.0)
    if mode == "nearest":
        return tap(np.rint(px).astype(np.int64), np.rint(py).astype(np.int64))
    x0, y0 = np.floor(px), np.floor(py)
    wx, wy = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return (tap(x0, y0) * ((1 - wy) * (1 - wx)) + tap(x0 + 1, y0) * ((1 - wy) * wx)
            + tap(x0, y0 + 1) * (wy * (1 - wx)) + tap(x0 + 1, y0 + 1) * (wy * wx))


def terms(imgs, fov, theta, phi, out_hw, mode, feather):
    """Per view: (p2e(img_i) (C, H, W), p2e(tent_i) (H, W)), float64."""
    m, _, h, w = imgs.shape
    tw = tent_image(h, w, feather)[None]
    res = []
    for i in range(m):
        u, v, mask = G.p2e_grid(h, w, float(fov[i]), float(theta[i]), float(phi[i]), out_hw[0], out_hw[1])
        res.append((sample(imgs[i], u, v, mode) * mask, sample(tw, u, v, mode)[0] * mask))
    return res


def mp2e(imgs, fov, theta, phi, out_hw, mode="bilinear", feather="horizontal", fill=255.0):
    """imgs (m, C, h, w) -> (out (C, H, W), summed weight (H, W)), float64."""
    num = np.zeros((imgs.shape[1],) + tuple(out_hw))
    den = np.zeros(tuple(out_hw))
    for img, wgt in terms(imgs, fov, theta, phi, out_hw, mode, feather):
        num += img * wgt
        den += wgt
    zero = den == 0
    return np.where(zero[None], fill, num / np.where(zero, 1.0, den)[None]), den
