"""The geometry kernels of pf_geometry.hip (grids, nearest indices, remap, EPA tables and their tile flags) away from the
benchmark cameras: any field of view, yaw outside one turn and fractional, pitch up to the poles, non-square views, camera
counts on both sides of the 12-camera launch batches, hand-made sample positions on every border, and tables whose sides are
no multiple of the 32 x 32 flag tile -- also as the attention kernel reads them.

References: tests/golden/geometry_cameras.npz (the reference's own answers, tools/make_golden_geometry.py) and
oracle/geometry.py, which tests/test_oracle_vs_reference.py pins to that fixture bit for bit for the same cameras.
Needs an MI355X: `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_within_one_ulp, golden, rel_l2
from oracle import geometry as G
from oracle import third_party as tp
from test_gpu_kernels import TOL, attn_ref, check, q16, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"

EDGE_CAMERAS = ((90, 0, 0), (90, 0, 90), (90, 0, -90), (90, 180, 0), (90, 360, 0),
                (90, -180, 45), (120, 359.999, 89.9), (60, 360 / 7, 0), (150, 12.5, -30), (20, 270, 10))
E2P_SIZES = ((16, 32, 16, 16), (32, 64, 12, 20), (17, 33, 9, 7), (64, 128, 32, 32))        # (eh, ew, h, w)
P2E_SIZES = ((16, 16, 16, 32), (12, 20, 32, 64), (9, 7, 17, 33))                           # (ph, pw, H, W)
P2E_INDEX_SIZES = P2E_SIZES[:2]        # at (9,7 | 17,33) the odd linspace counts put 713 of 19074 visible entries on a tie
MASK_SETS = (("cams5", (8, 8, 8, 16)), ("cams5", (6, 10, 8, 16)), ("cams5", (4, 4, 4, 8)), ("first13", (4, 4, 4, 8)))
TIE_PX = 1e-4                          # nearest: a sample position this close to x.5 may round either way
TIE_CAP = 0.01                         # ... for at most this share of the entries of a case
MASK_EPS = 1e-12                       # p2e mask: a comparison this close to equality (float64) may fall either way
MASK_CAP = 1e-3                        # ... for at most this share of the mask


def ops():
    from panfusion_amd import ops as o
    return o


def camera_list():
    """(34, 3) float64 rows (FoV, theta, phi) in degrees: 24 seeded random cameras, then the ten edge cameras
    (copy of tools/make_golden_geometry.py:camera_list; test_camera_list_is_the_fixtures checks it against the fixture)."""
    rng = np.random.default_rng(7)
    fov = np.round(rng.uniform(35, 130, 24), 3)                  # three draws of 24, in this order
    theta = np.round(rng.uniform(-400, 760, 24), 3)
    phi = np.round(rng.uniform(-90, 90, 24), 3)
    return np.concatenate([np.stack([fov, theta, phi], axis=1), np.array(EDGE_CAMERAS, dtype=np.float64)])


CAMS = camera_list()


@pytest.fixture(scope="module")
def geo():
    return golden("geometry_cameras.npz")


@functools.lru_cache(maxsize=None)
def oracle_e2p(size):
    """float64 (map_x, map_y, lon, lat), each (34, h, w), of the oracle for the camera list; computed once, never modified."""
    eh, ew, h, w = size
    maps = [G.e2p_grid(eh, ew, f, t, p, h, w) + G.pers_lonlat(f, t, p, h, w) for f, t, p in CAMS]
    return tuple(np.stack([m[k] for m in maps]) for k in range(4))


@functools.lru_cache(maxsize=None)
def oracle_p2e(size):
    """float64 (u, v), bool mask and the pixels the oracle cannot decide (mask_margin) for the camera list."""
    ph, pw, H, W = size
    u, v, mask, margin = [], [], [], []
    for f, t, p in CAMS:
        a = G.p2e_grid(ph, pw, f, t, p, H, W)
        u.append(a[0]), v.append(a[1]), mask.append(a[2])
        margin.append(mask_margin(ph, pw, f, t, p, H, W))
    return np.stack(u), np.stack(v), np.stack(mask), np.stack(margin)


def mask_margin(ph, pw, fov, theta, phi, H, W):
    """Where the float64 oracle cannot decide a pixel of p2e.py:36-47: bool (2, H, W), [0] for the visibility mask (x > 0 and
    -w_len < y / x < w_len and -h_len < z / x < h_len), [1] for the maps (the four window comparisons alone).  A pixel is
    undecided when a comparison lies within MASK_EPS of equality and every comparison that does not is true -- a near-equality
    next to a clearly false comparison (the pole rows of an unpitched camera: x = 6e-17 cos(lon), z / x = 1e16) decides nothing."""
    x, yy, zz, w_len, h_len = G.p2e_view_rays(ph, pw, fov, theta, phi, H, W)
    with np.errstate(invalid="ignore"):
        holds = np.stack([x > 0, -w_len < yy, yy < w_len, -h_len < zz, zz < h_len])
        near = np.stack([np.abs(x), np.abs(yy + w_len), np.abs(yy - w_len), np.abs(zz + h_len), np.abs(zz - h_len)]) <= MASK_EPS
    undecided = lambda s: near[s].any(0) & (holds[s] | near[s]).all(0)
    return np.stack([undecided(slice(0, 5)), undecided(slice(1, 5))])


def near_tie(coord_f64, size):
    pos = G.sample_position_f32(coord_f64, size).astype(np.float64)
    return np.abs(pos - np.floor(pos) - 0.5) <= TIE_PX


def check_indices(name, got, map_x, map_y, sh, sw):
    """`got` against G.nearest_indices of the float64 oracle maps: equal wherever the oracle's fp32 sample position is farther
    than TIE_PX from a half-integer on both axes; on a tie, one of the neighbouring candidates.  Returns the excluded count."""
    want = G.nearest_indices(map_x, map_y, sh, sw)
    tx, ty = near_tie(map_x, sw), near_tie(map_y, sh)
    tie = tx | ty
    bad = (got != want) & ~tie
    assert not bad.any(), "%s: %d of %d indices differ away from a tie" % (name, bad.sum(), bad.size)
    px, py = (G.sample_position_f32(m, s).astype(np.float64) for m, s in ((map_x, sw), (map_y, sh)))
    ok = np.zeros(got.shape, bool)
    for dx in (0, 1):
        for dy in (0, 1):
            cx = np.where(tx, np.floor(px) + dx, np.rint(px)).astype(np.int64)
            cy = np.where(ty, np.floor(py) + dy, np.rint(py)).astype(np.int64)
            inb = (cx >= 0) & (cx < sw) & (cy >= 0) & (cy < sh)
            ok |= got == np.where(inb, cy * sw + cx, -1)
    assert ok[tie].all(), "%s: %d indices on a tie are neither neighbour" % (name, (~ok[tie]).sum())
    share = tie.mean()
    print("\n%s: %d of %d entries within %g px of a tie (%.3f %%)" % (name, tie.sum(), tie.size, TIE_PX, 100 * share))
    assert share <= TIE_CAP, (name, share)
    return int(tie.sum())


def check_mask(name, got_mask, want_mask, undecided):
    """Visibility mask identical to the reference's except where the float64 comparison that decides it lies within MASK_EPS of
    equality (mask_margin, stacked over the cameras).  Returns the pixels whose mask or map entries may differ."""
    loose, loose_maps = undecided[:, 0], undecided[:, 0] | undecided[:, 1]
    diff = got_mask != want_mask
    print("\n%s: %d of %d mask pixels differ (tolerated); the oracle leaves %d (mask) / %d (maps) within %g of a tie"
          % (name, diff.sum(), diff.size, loose.sum(), loose_maps.sum(), MASK_EPS))
    assert not (diff & ~loose).any(), "%s: %d mask pixels differ away from a tie" % (name, (diff & ~loose).sum())
    assert diff.mean() <= MASK_CAP, (name, diff.mean())
    return loose_maps


def flipped_window(loose, gu, gv, wu, wv):
    """Of the pixels the oracle cannot decide, those where the kernel decided the window test the other way: one side wrote
    the (0, 0) of an invisible pixel, the other a position.  Only these are exempt from the comparison of the maps."""
    flipped = loose & (((gu == 0) & (gv == 0)) != ((wu == 0) & (wv == 0)))
    assert flipped.mean() <= MASK_CAP, flipped.mean()
    return flipped


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def test_camera_list_is_the_fixtures(geo):
    assert CAMS.shape == (34, 3) and np.array_equal(CAMS, geo["cams"])


# ------------------------------------------------------------------------------------ (a) grids, (b) nearest indices
@pytest.mark.parametrize("size", E2P_SIZES)
def test_e2p_grid_and_indices_all_cameras(geo, size):
    eh, ew, h, w = size
    mx, my, ll = ops().e2p_grid(CAMS[:, 0], CAMS[:, 1], CAMS[:, 2], eh, ew, h, w, DEV, want_lonlat=True)
    wx, wy, lon, lat = oracle_e2p(size)
    if size == (17, 33, 9, 7):                                   # (the full maps of the reference at the smallest size)
        assert np.array_equal(wx, geo["e2p_maps_17x33_9x7"][:, 0]) and np.array_equal(wy, geo["e2p_maps_17x33_9x7"][:, 1])
    assert_within_one_ulp(mx.cpu().numpy(), wx.astype(np.float32))
    assert_within_one_ulp(my.cpu().numpy(), wy.astype(np.float32))
    err = np.abs(ll.cpu().numpy().astype(np.float64) - np.stack([lon, lat], axis=-1)).max()
    assert err <= 1e-6, err
    idx = ops().nearest_indices(mx, my, eh, ew).cpu().numpy()
    check_indices("e2p %s" % (size,), idx, wx, wy, eh, ew)


@pytest.mark.parametrize("size", P2E_SIZES)
def test_p2e_grid_mask_and_indices_all_cameras(geo, size):
    ph, pw, H, W = size
    key = "%dx%d_%dx%d" % size
    mu, mv, mask = ops().p2e_grid(CAMS[:, 0], CAMS[:, 1], CAMS[:, 2], ph, pw, H, W, DEV)
    wu, wv, wmask, margin = oracle_p2e(size)
    ref_mask = np.unpackbits(geo["p2e_mask_" + key])[:34 * H * W].reshape(34, H, W).astype(bool)
    assert np.array_equal(wmask, ref_mask)
    if size == (9, 7, 17, 33):
        assert np.array_equal(wu, geo["p2e_maps_9x7_17x33"][:, 0]) and np.array_equal(wv, geo["p2e_maps_9x7_17x33"][:, 1])
    loose = check_mask("p2e %s" % (size,), mask.cpu().numpy().astype(bool), ref_mask, margin)
    gu, gv = mu.cpu().numpy(), mv.cpu().numpy()
    wu32, wv32 = wu.astype(np.float32), wv.astype(np.float32)
    flipped = flipped_window(loose, gu, gv, wu32, wv32)
    print("p2e %s: %d map entries exempt (window test undecided and decided the other way)" % (size, flipped.sum()))
    assert_within_one_ulp(np.where(flipped, wu32, gu), wu32)
    assert_within_one_ulp(np.where(flipped, wv32, gv), wv32)
    if size in P2E_INDEX_SIZES:
        idx = ops().nearest_indices(mu, mv, ph, pw).cpu().numpy()
        idx = np.where(flipped, G.nearest_indices(wu, wv, ph, pw), idx)
        check_indices("p2e %s" % (size,), idx, wu, wv, ph, pw)
        print("p2e %s: %d of them visible" % (size, (near_tie(wu, pw) | near_tie(wv, ph))[wmask].sum()))


# ------------------------------------------------------------------------------------ (c) camera batching
@functools.lru_cache(maxsize=None)
def single_camera_grids():
    """The 34 single-camera launches of both grid kernels at the smallest sizes, stacked (device tensors, never modified)."""
    eh, ew, h, w = E2P_SIZES[2]
    ph, pw, H, W = P2E_SIZES[2]
    e = [ops().e2p_grid(c[0:1], c[1:2], c[2:3], eh, ew, h, w, DEV, want_lonlat=True) for c in CAMS]
    p = [ops().p2e_grid(c[0:1], c[1:2], c[2:3], ph, pw, H, W, DEV) for c in CAMS]
    return tuple(torch.cat([a[k] for a in e]) for k in range(3)), tuple(torch.cat([a[k] for a in p]) for k in range(3))


@pytest.mark.parametrize("n", [1, 11, 12, 13, 24, 25, 34])
def test_grid_camera_batches_equal_single_camera_calls(n):
    eh, ew, h, w = E2P_SIZES[2]
    ph, pw, H, W = P2E_SIZES[2]
    se, sp = single_camera_grids()
    got = ops().e2p_grid(CAMS[:n, 0], CAMS[:n, 1], CAMS[:n, 2], eh, ew, h, w, DEV, want_lonlat=True)
    for name, a, b in zip(("map_x", "map_y", "lonlat"), got, se):
        assert a.shape[0] == n and torch.equal(bits(a), bits(b[:n])), "e2p %s, %d cameras" % (name, n)
    got = ops().p2e_grid(CAMS[:n, 0], CAMS[:n, 1], CAMS[:n, 2], ph, pw, H, W, DEV)
    for name, a, b in zip(("map_u", "map_v", "mask"), got, sp):
        assert a.shape[0] == n and torch.equal(bits(a), bits(b[:n])), "p2e %s, %d cameras" % (name, n)


def tile_flags(table):
    """'Any non-zero in the 32 x 32 tile' of a table zero-padded up to multiples of 32."""
    nq, nk = table.shape
    pad = torch.zeros((nq + 31) // 32 * 32, (nk + 31) // 32 * 32)
    pad[:nq, :nk] = table.cpu()
    return pad.reshape(pad.shape[0] // 32, 32, pad.shape[1] // 32, 32).abs().amax((1, 3)) > 0


@pytest.mark.parametrize("m", [1, 12, 13])
def test_epa_table_camera_batches_equal_single_camera_calls(m):
    ph, pw, eh, ew = 4, 4, 4, 8
    P = ph * pw
    be, bp, fe, fp = ops().epa_tables(CAMS[:m, 0], CAMS[:m, 1], CAMS[:m, 2], ph, pw, eh, ew, DEV)
    assert be.shape == (eh * ew, m * P) and bp.shape == (m * P, eh * ew)
    for i in range(m):
        b1, p1, _, _ = ops().epa_tables(CAMS[i:i + 1, 0], CAMS[i:i + 1, 1], CAMS[i:i + 1, 2], ph, pw, eh, ew, DEV)
        assert torch.equal(bits(be[:, i * P:(i + 1) * P]), bits(b1)), "bias_e, camera %d of %d" % (i, m)
        assert torch.equal(bits(bp[i * P:(i + 1) * P]), bits(p1)), "bias_p, camera %d of %d" % (i, m)
    assert torch.equal(fe.cpu().bool(), tile_flags(be)) and torch.equal(fp.cpu().bool(), tile_flags(bp))


# ------------------------------------------------------------------------------------ (d) remap on hand-made maps
def hand_made_maps(map_batch, hs, ws, ho, wo, seed):
    """fp32 maps (map_batch, ho, wo): positions drawn from [-1.5, size + 0.5] on both axes, half of the entries (at seeded
    places) overwritten with pairs of exact edge positions: first / last pixel, half a pixel and a whole pixel outside on either
    side, x.5 with an even and with an odd integer part, an exact integer."""
    g = torch.Generator().manual_seed(seed)
    n = map_batch * ho * wo
    mx = torch.rand(n, generator=g) * (ws + 2.0) - 1.5
    my = torch.rand(n, generator=g) * (hs + 2.0) - 1.5
    edge = lambda s: [0.0, s - 1.0, -0.5, s - 0.5, -1.0, float(s), 2.5, 3.5, 4.0]
    ex, ey = edge(ws), edge(hs)
    pairs = [(ex[i], ey[(i + j) % 9]) for j in range(9) for i in range(9)][:n // 2]
    at = torch.randperm(n, generator=g)[:len(pairs)]
    mx[at] = torch.tensor([p[0] for p in pairs])
    my[at] = torch.tensor([p[1] for p in pairs])
    mask = (torch.rand(n, generator=g) > 0.3).to(torch.uint8)
    return mx.reshape(map_batch, ho, wo), my.reshape(map_batch, ho, wo), mask.reshape(map_batch, ho, wo)


def ulp16(x, dtype):
    """One unit in the last place of ``dtype`` at the magnitude of the fp32 values x."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.frexp(x.abs())[1] - 1                              # |x| = 1.f * 2^e
    e = torch.where(x == 0, torch.full_like(e, emin), e)
    return torch.ldexp(torch.ones_like(x), e.clamp_min(emin) - mant)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("map_batch", [1, 3])
def test_remap_hand_made_maps(dtype, mode, with_mask, map_batch):
    B, C, hs, ws, ho, wo = 3, 5, 7, 11, 6, 9
    src = rnd(B, C, hs, ws, seed=51).to(dtype)
    mx, my, mask = hand_made_maps(map_batch, hs, ws, ho, wo, seed=52 + map_batch)
    want = tp.remap(src.float(), mx, my, align_corners=True, mode=mode)
    if with_mask:
        want = want * mask[:, None]
    got = ops().remap(src.to(DEV), mx.to(DEV), my.to(DEV), mode, mask=mask.to(DEV) if with_mask else None)
    assert got.dtype == dtype and got.shape == (B, C, ho, wo)
    got = got.float().cpu()
    if mode == "nearest":                                        # a pure gather
        bad = got != want
        assert not bad.any(), "%d of %d differ, first at %s" % (bad.sum(), bad.numel(), bad.nonzero()[0].tolist())
        return
    err = rel_l2(got, want)
    print("\nremap bilinear %s mask %d map_batch %d: rel-L2 %.3e, max abs %.3e" % (dtype, with_mask, map_batch, err, float((got - want).abs().max())))
    assert err <= (1e-5 if dtype == torch.float32 else TOL[dtype]), err
    if dtype == torch.float32:
        # four products and three sums in fp32, whose order and contraction may differ: a few roundings at the magnitude of
        # the largest source value (2^-21 |src|_max allows eight half-ulp roundings)
        bound = torch.full_like(want, 1e-6 + 2.0 ** -21 * float(src.float().abs().max()))
    else:
        bound = ulp16(want, dtype) + 1e-6
    worst = (got - want).abs() - bound
    assert float(worst.max()) <= 0, "element %s off by %.3e (bound %.3e)" % (
        np.unravel_index(int(worst.argmax()), worst.shape), float((got - want).abs().flatten()[worst.argmax()]), float(bound.flatten()[worst.argmax()]))


# ------------------------------------------------------------------------------------ (e) API level
def api():
    from panfusion_amd.external.Perspective_and_Equirectangular import e2p, p2e
    return e2p, p2e


def check_e2p_api(name, x, cams, out_hw, cams_oracle=None):
    """e2p of the product against G.e2p, both modes; the cameras in the form given (tensor, list or scalars)."""
    e2p, _ = api()
    b, _, eh, ew = x.shape
    oc = cams if cams_oracle is None else cams_oracle
    per = G._per_sample(b, *oc)
    maps = [G.e2p_grid(eh, ew, f, t, p, out_hw[0], out_hw[1]) for f, t, p in per]
    tie = np.stack([near_tie(m[0], ew) | near_tie(m[1], eh) for m in maps])
    print("\n%s: %d of %d pixels within %g px of a tie" % (name, tie.sum(), tie.size, TIE_PX))
    assert tie.mean() <= TIE_CAP
    keep = torch.from_numpy(~tie)[:, None]
    out = {}
    for mode in ("nearest", "bilinear"):
        got = e2p(x.to(DEV), *cams, out_hw, mode=mode).cpu()
        want = G.e2p(x, *oc, out_hw, mode=mode)
        assert got.shape == want.shape
        if mode == "nearest":
            assert torch.equal(got * keep, want * keep), "%s nearest: %d differ" % (name, ((got != want) & keep).sum())
        else:
            check(name + " bilinear", got, want, 1e-5)
        out[mode] = got
    return out


def check_p2e_api(name, y, cams, out_hw, cams_oracle=None):
    _, p2e = api()
    b, _, ph, pw = y.shape
    oc = cams if cams_oracle is None else cams_oracle
    per = G._per_sample(b, *oc)
    maps = [G.p2e_grid(ph, pw, f, t, p, out_hw[0], out_hw[1]) for f, t, p in per]
    margin = np.stack([mask_margin(ph, pw, f, t, p, out_hw[0], out_hw[1]) for f, t, p in per])
    tie = np.stack([near_tie(m[0], pw) | near_tie(m[1], ph) for m in maps])
    print("\n%s: %d of %d pixels within %g px of a tie" % (name, tie.sum(), tie.size, TIE_PX))
    assert tie.mean() <= TIE_CAP
    out = {}
    for mode in ("nearest", "bilinear"):
        ge, gm = p2e(y.to(DEV), *cams, out_hw, mode=mode)
        we, wm = G.p2e(y, *oc, out_hw, mode=mode)
        ge, gm = ge.cpu(), gm.cpu()
        assert ge.shape == we.shape and gm.shape == wm.shape and gm.dtype == torch.bool
        check_mask(name, gm[:, 0].numpy(), wm[:, 0].numpy(), margin)
        keep = gm == wm                                          # (a pixel whose window test flips is visible on one side only)
        if mode == "nearest":
            keep = keep & torch.from_numpy(~tie)[:, None]
            assert torch.equal(ge * keep, we * keep), "%s nearest: %d differ" % (name, ((ge != we) & keep).sum())
        else:
            check(name + " bilinear", ge * keep, we * keep, 1e-5)
        out[mode] = (ge, gm)
    return out


def test_api_camera_containers_and_non_square_view():
    """34 cameras, one per sample, 32x64 panorama <-> 12x20 views (hfov = h / w * fov).  The same cameras as a float64 tensor and
    as a list, and the float32-rounded cameras as a float32 tensor, as that tensor widened to float64 and as a list, must give
    the same bits: the container does not matter, only the values."""
    x, y = rnd(34, 3, 32, 64, seed=61), rnd(34, 3, 12, 20, seed=62)
    c64 = [torch.tensor(CAMS[:, k]) for k in range(3)]
    c32 = [c.float() for c in c64]
    forms = {"float64 tensor": (c64, c64), "list": ([c.tolist() for c in c64], c64),
             "float32 tensor": (c32, c32), "float32 widened": ([c.double() for c in c32], c32), "float32 list": ([c.tolist() for c in c32], c32)}
    res = {k: (check_e2p_api("e2p, " + k, x, cams, (12, 20), oc), check_p2e_api("p2e, " + k, y, cams, (32, 64), oc)) for k, (cams, oc) in forms.items()}
    for a, b in (("float64 tensor", "list"), ("float32 tensor", "float32 widened"), ("float32 tensor", "float32 list")):
        for mode in ("nearest", "bilinear"):
            assert torch.equal(res[a][0][mode], res[b][0][mode]), (a, b, mode)
            assert torch.equal(res[a][1][mode][0], res[b][1][mode][0]) and torch.equal(res[a][1][mode][1], res[b][1][mode][1]), (a, b, mode)


def test_api_single_photo_into_a_panorama():
    """The call of KnownRegion.from_view: one 24x40 photo, FoV 70 at (33.3, -60), into a 32x64 panorama."""
    y = rnd(1, 3, 24, 40, seed=63)
    out = check_p2e_api("photo", y, ([70], [33.3], [-60]), (32, 64))
    covered = out["bilinear"][1]
    assert covered.shape == (1, 1, 32, 64) and 0 < int(covered.sum()) < 32 * 64


def test_api_scalar_camera_broadcast():
    """All three scalars: one grid for the batch (e2p.py:65-66), which is pf_remap's map_batch = 1, in p2e with its mask."""
    x, y = rnd(3, 3, 16, 32, seed=64), rnd(3, 3, 10, 14, seed=65)
    check_e2p_api("scalar e2p", x, (75.5, 412.3, -35.25), (10, 14))
    out = check_p2e_api("scalar p2e", y, (75.5, 412.3, -35.25), (16, 32))
    assert out["nearest"][1].shape == (1, 1, 16, 32)


# ------------------------------------------------------------------------------------ (f) EPA tables, (g) into attention
def mask_set(geo, which, shape):
    c = geo["cams5"] if which == "cams5" else geo["cams"][:13]
    name = "%s_%dx%d_%dx%d" % ((which,) + shape)
    return c, torch.from_numpy(geo["masks_%s_pers" % name]), torch.from_numpy(geo["masks_%s_equi" % name])


@pytest.mark.parametrize("which,shape", MASK_SETS)
def test_epa_tables_vs_reference_and_ragged_flags(geo, which, shape):
    """m * P = 80, 208 (P = 16) and 300 (P = 60): no multiple of 32, the last flag tile is partial."""
    ph, pw, eh, ew = shape
    c, pers, equi = mask_set(geo, which, shape)
    m, E, P = len(c), eh * ew, ph * pw
    be, bp, fe, fp = ops().epa_tables(c[:, 0], c[:, 1], c[:, 2], ph, pw, eh, ew, DEV)
    want_e = pers.reshape(m, E, P).permute(1, 0, 2).reshape(E, m * P) + 1
    want_p = equi.reshape(m * P, E) + 1
    ee, ep = float((be.cpu() - want_e).abs().max()), float((bp.cpu() - want_p).abs().max())
    print("\nEPA tables %s %s: max abs error %.3e / %.3e" % (which, shape, ee, ep))
    # (2e-5: supports may differ by entries of magnitude < 2e-5, a bilinear weight that is exactly 0 on one side)
    assert ee <= 2e-5 and ep <= 2e-5, (ee, ep)
    for bias, flags in ((be, fe), (bp, fp)):
        assert float(bias.min()) >= 0 and float(bias.max()) <= 2 + 1e-6
        assert flags.shape == ((bias.shape[0] + 31) // 32, (bias.shape[1] + 31) // 32)
        assert torch.equal(flags.cpu().bool(), tile_flags(bias))
    again = ops().epa_tables(c[:, 0], c[:, 1], c[:, 2], ph, pw, eh, ew, DEV)
    for a, b in zip((be, bp, fe, fp), again):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("shape", [(4, 4, 4, 8), (6, 10, 8, 16)])
@pytest.mark.parametrize("direction", ["pano_queries", "view_queries"])
def test_attention_reads_ragged_epa_tables(geo, direction, shape):
    """E = 32 panorama pixels against m * P = 80 view pixels: the attention kernel with the table's own bias, flags and
    flags_ld = 3 (resp. 1), the last key tile (resp. query tile) partial; every tile of these small tables is flagged.
    E = 128 against m * P = 300: flags_ld = 10 (resp. 4), the last of ten tiles holds 12 keys (resp. queries), and some
    of the tiles are empty (13 resp. 3 of 40), so that a flag read from the wrong place drops or adds a tile of bias."""
    ph, pw, eh, ew = shape
    c = geo["cams5"]
    E, mP = eh * ew, len(c) * ph * pw
    be, bp, fe, fp = ops().epa_tables(c[:, 0], c[:, 1], c[:, 2], ph, pw, eh, ew, DEV)
    bias, flags = (be, fe) if direction == "pano_queries" else (bp, fp)
    nq, nk = bias.shape
    assert (nq, nk) == ((E, mP) if direction == "pano_queries" else (mP, E)) and flags.shape == ((nq + 31) // 32, (nk + 31) // 32)
    assert mP % 32 != 0 and bool(flags[-1, -1]) and float(bias.max()) > 1.5
    if shape == (6, 10, 8, 16):
        assert 0 < float((flags == 0).float().mean()) < 0.5
    B, H, D, dtype = 2, 2, 32, torch.float16
    Cq = H * D
    q, qf = q16(rnd(B, nq, Cq, seed=71), dtype)
    k, kf = q16(rnd(B, nk, Cq, seed=72), dtype)
    v, vf = q16(rnd(B, nk, Cq, seed=73), dtype)
    ld = (nk + 31) // 32 * 32
    vt = torch.full((B, Cq, ld), float("nan"), dtype=dtype, device=DEV)     # padding must never be read as data
    vt[:, :, :nk] = v.transpose(1, 2)
    call = lambda fl: ops().attention(q, k, vt, B, H, D, nq, nk, q_ld=Cq, k_ld=Cq, vt_ld=ld, q_bs=nq * Cq, k_bs=nk * Cq, vt_bs=Cq * ld,
                                      bias=bias, flags=fl)
    out = call(flags)
    check("attention with ragged tables", out, attn_ref(qf, kf, vf, H, D ** -0.5, bias.cpu()), 2.5 * TOL[dtype])
    check("table flags vs all-ones flags", out, call(torch.ones_like(flags)), 1.5 * TOL[dtype])
