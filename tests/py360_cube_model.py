"""numpy-only float64 statement of the cube-map conversions (reference ``external/py360convert/e2c.py``, ``c2e.py``,
``utils.py:5-64,82-173``) and the per-element bounds of DESIGN.md 4.2.  TEST INFRASTRUCTURE: no scipy (the GPU
machine may not have it), never imported by the product.

Where the reference evaluates xyz2uv / uv2coor (e2c) and tan / cos / sin (c2e) in float32, this model and the kernels
evaluate them in float64 from the same float32-rounded inputs.  numpy's float32 transcendentals are not correctly
rounded, so the reference's coordinates differ from these by ``eps_meas`` (a few float32 ulps, stored per shape in
tests/golden/py360_cube.npz); the tests allow eps = 4 eps_meas and bound what that does to every output element.
"""
import numpy as np

from oracle.py360 import _wrap_coord, _wrap_index

EPS_FACTOR = 4.0          # 2 (another numpy build erring the other way) x 2 (maximum error and steepest gradient apart)
TIE_MODEL = 1e-9          # kernel against this model: same tie radius as the e2p tests
NEAREST_CAP = 0.15        # share of pixels a nearest-mode case may excuse
TWO_VALUED_CAP = 0.05     # share of uint8 bilinear elements with two admissible values

E2C_SHAPES = ((32, 64, 24), (33, 66, 17), (47, 95, 31))        # (H, W, face_w)
C2E_SHAPES = ((32, 64, 24), (16, 32, 8), (31, 56, 13))         # (h, w, face_w)


# ------------------------------------------------------------------------------------------------ coordinates
def _f32_linspace(a, b, n):
    return np.linspace(a, b, num=n, dtype=np.float32).astype(np.float64)


def e2c_coords(H, W, face_w):
    """-> (coor_x, coor_y) float64 [face_w, 6 face_w]: utils.py xyzcube in float32, xyz2uv + uv2coor in float64."""
    rng = _f32_linspace(-0.5, 0.5, face_w)
    gx, gy = np.meshgrid(rng, -rng)
    half = np.full_like(gx, 0.5)
    # per face (x, y, z): F z=+.5, R x=+.5, B z=-.5, L x=-.5, U y=+.5, D y=-.5
    faces = ((gx, gy, half), (half, gy, gx), (gx, gy, -half), (-half, gy, gx), (gx, half, gy), (gx, -half, gy))
    x, y, z = (np.concatenate([f[k] for f in faces], axis=1) for k in range(3))
    lon = np.arctan2(x, z)
    lat = np.arctan2(y, np.sqrt(x ** 2 + z ** 2))
    return (lon / (2 * np.pi) + 0.5) * W - 0.5, (-lat / np.pi + 0.5) * H - 0.5


def facetype(h, w):
    """utils.py:47-64 equirect_facetype, restated per pixel: side face from the column, U above the ceiling row of the
    column's quarter-period, D below the mirrored one (D wins)."""
    idx = np.linspace(-np.pi, np.pi, w // 4) / 4
    ceil_rows = h // 2 - np.round(np.arctan(np.cos(idx)) * h / np.pi).astype(int)
    j = (np.arange(w) - 3 * w // 8) % w
    rows = np.arange(h)[:, None]
    ceil = ceil_rows[j % (w // 4)][None, :]
    tp = np.broadcast_to(j // (w // 4), (h, w)).copy()
    tp[np.broadcast_to(rows < ceil, (h, w))] = 4
    tp[np.broadcast_to(rows >= h - ceil, (h, w))] = 5
    return tp


def c2e_coords(h, w, face_w):
    """-> (tp, coor_x, coor_y): c2e.py:29-57 in float64 from the float32 equirect_uvgrid values."""
    u = np.broadcast_to(_f32_linspace(-np.pi, np.pi, w)[None, :], (h, w))
    v = np.broadcast_to((_f32_linspace(np.pi, -np.pi, h) / 2)[:, None], (h, w))
    tp = facetype(h, w)
    a = u - np.pi * np.minimum(tp, 3) / 2
    side_x, side_y = 0.5 * np.tan(a), -0.5 * np.tan(v) / np.cos(a)
    c = 0.5 * np.tan(np.pi / 2 - np.where(tp == 4, v, np.abs(v)))
    cap_x, cap_y = c * np.sin(u), c * np.cos(u)
    cx = np.where(tp < 4, side_x, cap_x)
    cy = np.where(tp < 4, side_y, np.where(tp == 4, cap_y, -cap_y))
    return tp, (np.clip(cx, -0.5, 0.5) + 0.5) * face_w, (np.clip(cy, -0.5, 0.5) + 0.5) * face_w


# ------------------------------------------------------------------------------------------------ padded sources
def pad_equirec(img):
    """utils.py:128-130: [H, W, C] -> float64 [1, H + 2, W, C] (rows H, H + 1: last and first row rolled by W // 2)."""
    W = img.shape[1]
    return np.concatenate([img, np.roll(img[[-1]], W // 2, 1), np.roll(img[[0]], W // 2, 1)], 0).astype(np.float64)[None]


def pad_cube(cube_h):
    """utils.py:136-171: horizon [F, 6F, C] -> float64 [6, F + 2, F + 2, C], the array sample_cubefaces hands to
    map_coordinates: flips, then two rows after row F - 1, then two columns after column F - 1."""
    F = cube_h.shape[0]
    g = np.stack([cube_h[:, i * F:(i + 1) * F] for i in range(6)]).astype(np.float64)
    g[1], g[2], g[4] = g[1, :, ::-1].copy(), g[2, :, ::-1].copy(), g[4, ::-1].copy()
    rows = [(g[5, 0], g[4, -1]), (g[5, :, -1], g[4, ::-1, -1]), (g[5, -1, ::-1], g[4, 0, ::-1]),
            (g[5, ::-1, 0], g[4, :, 0]), (g[0, 0], g[2, 0, ::-1]), (g[2, -1, ::-1], g[0, -1])]
    e = np.concatenate([g, np.stack([np.stack(r) for r in rows])], axis=1)           # [6, F + 2, F, C]
    cols = np.zeros((6, F + 2, 2) + e.shape[3:])
    for f in range(4):
        cols[f, :, 0], cols[f, :, 1] = e[(f + 1) % 4, :, 0], e[(f + 3) % 4, :, -1]
    cols[4, 1:-1, 0], cols[4, 1:-1, 1] = e[1, 0, ::-1], e[3, 0]
    cols[5, 1:-1, 0], cols[5, 1:-1, 1] = e[1, -2], e[3, -2, ::-1]
    return np.concatenate([e, cols], axis=2)


# ------------------------------------------------------------------------------------------------ sampling
def _tap(P, face, iy, ix):
    return P[face, _wrap_index(iy, P.shape[1]), _wrap_index(ix, P.shape[2])]


def sample(P, face, cy, cx, order):
    """map_coordinates(P[..., ch], [face, cy, cx], order, mode='wrap') for every channel, unrounded float64.  The face
    coordinate is an integer: its second tap has weight 0."""
    y, x = _wrap_coord(cy, P.shape[1]), _wrap_coord(cx, P.shape[2])
    if order == 0:
        return _tap(P, face, np.floor(y + 0.5).astype(np.int64), np.floor(x + 0.5).astype(np.int64))
    y0, x0 = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)
    fy, fx = (y - y0)[..., None], (x - x0)[..., None]
    acc = 0.0
    for ky, wy in enumerate((1 - fy, fy)):
        for kx, wx in enumerate((1 - fx, fx)):
            acc = acc + _tap(P, face, y0 + ky, x0 + kx) * wy * wx
    return acc


def neighbourhood(P, face, cy, cx):
    """-> (Gx, Gy, local range) per output element: over the 3 x 3 cells around the sampling position (4 x 4 samples of
    the padded source, indices wrapped like the sampler's), the largest difference of horizontally / vertically
    adjacent samples and max - min."""
    y0 = np.floor(_wrap_coord(cy, P.shape[1])).astype(np.int64)
    x0 = np.floor(_wrap_coord(cx, P.shape[2])).astype(np.int64)
    blk = np.stack([np.stack([_tap(P, face, y0 + dy, x0 + dx) for dx in (-1, 0, 1, 2)]) for dy in (-1, 0, 1, 2)])
    gx = np.abs(np.diff(blk, axis=1)).max((0, 1))
    gy = np.abs(np.diff(blk, axis=0)).max((0, 1))
    return gx, gy, blk.max((0, 1)) - blk.min((0, 1))


def tie(shape_yx, cy, cx, radius):
    """Nearest mode: positions within ``radius`` of a half-integer on either axis (after the wrap)."""
    frac = lambda c: np.abs((c + 0.5) - np.round(c + 0.5))
    return (frac(_wrap_coord(cy, shape_yx[0])) <= radius) | (frac(_wrap_coord(cx, shape_yx[1])) <= radius)


def scipy_u8(t):
    """scipy's integer store: round half up, clamp."""
    return np.clip(np.where(t > 0, t + 0.5, 0.0), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ conversions
def e2c_setup(img, face_w):
    cx, cy = e2c_coords(img.shape[0], img.shape[1], face_w)
    return pad_equirec(img), np.zeros(cx.shape, np.int64), cy, cx


def c2e_setup(cube_h, h, w):
    tp, cx, cy = c2e_coords(h, w, cube_h.shape[0])
    return pad_cube(cube_h), tp, cy, cx


def e2c(img, face_w, order):
    """horizon cube map [face_w, 6 face_w, C] in img.dtype."""
    acc = sample(*e2c_setup(img, face_w), order)
    return scipy_u8(acc) if img.dtype == np.uint8 else acc.astype(img.dtype)


def c2e(cube_h, h, w, order):
    """[h, w, C] float64."""
    return sample(*c2e_setup(cube_h, h, w), order)


# ------------------------------------------------------------------------------------------------ bounds
def rounding(value, dtype):
    """r of the bilinear bound: 2 float32 ulps of the value, or 1e-12 |value| for float64."""
    if np.dtype(dtype) == np.float32:
        return 2.0 * np.spacing(np.abs(value).astype(np.float32)).astype(np.float64)
    return 1e-12 * np.abs(value)


def check(got, want, setup, order, eps, label=""):
    """``got`` against ``want`` under a coordinate uncertainty ``eps`` (pixels of the source), both in the dtype the
    conversion returns; ``setup`` is e2c_setup / c2e_setup of the input.  Asserts the bound on every element and the caps,
    returns the share of elements that were excused (nearest) or had two admissible values (uint8 bilinear).

    bilinear, float:  |got - want| <= eps (Gx + Gy) + r
    bilinear, uint8:  got and want each equal scipy's rounding of model - eps (Gx + Gy) or of model + eps (Gx + Gy)
    nearest:          equal, except within eps of a half-integer position, and there within the source's local range
    """
    P, face, cy, cx = setup
    assert got.shape == want.shape and got.dtype == want.dtype, (label, got.shape, want.shape, got.dtype, want.dtype)
    gx, gy, local = neighbourhood(P, face, cy, cx)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if order == 0:
        excused = np.broadcast_to(tie(P.shape[1:3], cy, cx, eps)[..., None], got.shape)
        bad = (diff != 0) & ~excused
        assert not bad.any(), "%s: %d of %d nearest samples differ outside ties" % (label, bad.sum(), bad.size)
        assert (diff <= local).all(), "%s: a tie differs by more than the source's local range" % label
        share = float(excused.mean())
        assert share <= NEAREST_CAP, "%s: %.1f %% of the pixels are ties" % (label, 100 * share)
        return share
    bound = eps * (gx + gy)
    if got.dtype == np.uint8:
        model = sample(P, face, cy, cx, 1)
        lo, hi = scipy_u8(model - bound), scipy_u8(model + bound)
        for name, a in (("got", got), ("want", want)):
            bad = (a != lo) & (a != hi)
            assert not bad.any(), "%s: %d of %d %s values outside the admissible pair" % (label, bad.sum(), bad.size, name)
        assert (diff <= local).all(), "%s: a two-valued element differs by more than the source's local range" % label
        share = float((lo != hi).mean())
        assert share <= TWO_VALUED_CAP, "%s: %.1f %% of the elements have two admissible values" % (label, 100 * share)
        return share
    bound = bound + rounding(want, got.dtype)
    bad = ~(diff <= bound)
    assert not bad.any(), "%s: %d of %d elements beyond eps (Gx + Gy) + r, worst excess %.3e" % (
        label, bad.sum(), bad.size, (diff - bound).max())
    return 0.0


def check_tight(got, setup, order, label="", whole_image=True):
    """A kernel against this model: nearest exact outside 1e-9 ties; uint8 exact outside positions where the unrounded
    value sits within 1e-9 (Gx + Gy) of a rounding step; float32 within 2 ulps; float64 within
    1e-9 (Gx + Gy) + 1e-12 |value|.  For a whole image the share of excused elements is capped as well (a chosen
    subset, such as the seam column, may consist of them)."""
    P, face, cy, cx = setup
    acc = sample(P, face, cy, cx, order)
    if order == 0:
        keep = ~np.broadcast_to(tie(P.shape[1:3], cy, cx, TIE_MODEL)[..., None], got.shape)
        assert keep.mean() > 0.8 or not whole_image, label
        want = scipy_u8(acc) if got.dtype == np.uint8 else acc.astype(got.dtype)
        bad = (got != want) & keep
        assert not bad.any(), "%s: %d of %d nearest samples differ from the model" % (label, bad.sum(), bad.size)
        return
    gx, gy, _ = neighbourhood(P, face, cy, cx)
    slack = TIE_MODEL * (gx + gy)
    if got.dtype == np.uint8:
        bad = (got != scipy_u8(acc - slack)) & (got != scipy_u8(acc + slack))
        assert not bad.any(), "%s: %d of %d uint8 values differ from the model" % (label, bad.sum(), bad.size)
        # (a sum lands on k + 1/2 where a weight is exactly 1/2: the centre row and column of an odd face, a few per mille)
        assert (scipy_u8(acc - slack) != scipy_u8(acc + slack)).mean() < 1e-2 or not whole_image, label
        return
    if got.dtype == np.float32:
        tol = 2.0 * np.spacing(np.abs(acc).astype(np.float32)).astype(np.float64) + slack
    else:
        tol = slack + 1e-12 * np.abs(acc)
    diff = np.abs(got.astype(np.float64) - acc)
    assert (diff <= tol).all(), "%s: worst excess over the model tolerance %.3e" % (label, (diff - tol).max())
