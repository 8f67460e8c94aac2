"""Pins oracle/*.py against the reference's OWN modules, through the answers tools/make_golden_refpins.py recorded from them
(oracle/ref_import.py) on the same seeded inputs: tests/golden/ref_pins.npz and tests/golden/ref_cfg1_call.npz.  What was
compared bit-exactly with the reference is compared with the SHA-256 digest of the reference's value (dtype-agnostic,
-0.0 == +0.0, as np.array_equal / torch.equal); what was compared to a tolerance is compared with the stored array."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import assert_within_one_ulp, cam4, golden, rel_l2
from oracle import geometry as G
from oracle import mvgen as MV
from oracle import sd2_unet as U

GRID_SIZES = ((64, 128, 64, 64), (32, 64, 32, 32), (16, 32, 16, 16), (8, 16, 8, 8), (128, 256, 64, 64))


@pytest.fixture(scope="module")
def ref():
    return golden("ref_pins.npz")


def digest(*arrays):
    """SHA-256 of the VALUES of a sequence of arrays (tools/make_golden_refpins.py:digest)."""
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.dtype.kind == "f":
            a = a.astype(np.float64) + 0.0
        elif a.dtype.kind in "iu":
            a = a.astype(np.int64)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def ico_deg(ref):
    return np.degrees(ref["ico_theta"]), np.degrees(ref["ico_phi"])


def test_random_sample_camera_same_draws(ref):
    """utils/pano.py:15-25 against the product's sampler under the same numpy seed."""
    from panfusion_amd.utils.pano import random_sample_camera
    np.random.seed(123)
    got = random_sample_camera(20)
    assert np.array_equal(got[0], ref["random_theta"]) and np.array_equal(got[1], ref["random_phi"])


def test_cameras(ref):
    b = G.icosahedron_cameras()
    assert np.array_equal(ref["ico_theta"], b[0]) and np.array_equal(ref["ico_phi"], b[1])
    b = G.horizon_cameras(8)
    assert np.array_equal(ref["horizon8_theta"], b[0]) and np.array_equal(ref["horizon8_phi"], b[1])


@pytest.mark.parametrize("rot", [0, 90, 180, 270])
def test_grids_bit_exact_all_benchmark_cameras(ref, rot):
    thd, phd = ico_deg(ref)
    t = [(thd[i] + rot) % 360 for i in range(20)]
    for k, (eh, ew, h, w) in enumerate(GRID_SIZES):
        e2p = digest(*[a for i in range(20) for a in G.e2p_grid(eh, ew, 90, t[i], phd[i], h, w)])
        assert np.array_equal(e2p, ref["grid_e2p_rot%d" % rot][k]), (eh, ew, h, w)
        p2e = digest(*[a for i in range(20) for a in G.p2e_grid(h, w, 90, t[i], phd[i], eh, ew)])
        assert np.array_equal(p2e, ref["grid_p2e_rot%d" % rot][k]), (eh, ew, h, w)


def test_remap_modes(ref):
    thd, phd = ico_deg(ref)
    cams = (torch.full((20,), 90), torch.tensor(thd), torch.tensor(phd))
    g = torch.Generator().manual_seed(31)
    x, y = torch.randn(20, 3, 16, 32, generator=g), torch.randn(20, 3, 16, 16, generator=g)
    for mode in ("nearest", "bilinear", None):
        assert np.array_equal(digest(G.e2p(x, *cams, (16, 16), mode=mode)), ref["e2p_%s" % mode]), mode
    assert np.array_equal(digest(*G.p2e(y, *cams, (16, 32))), ref["p2e"])
    # scalar camera broadcast (e2p.py:65-66)
    assert np.array_equal(digest(G.e2p(x, 90, 30.0, 10.0, (8, 8))), ref["e2p_scalar_camera"])


def test_masks_coords_pe(ref):
    thd, phd = ico_deg(ref)
    cams = {"FoV": torch.full((20,), 90), "theta": torch.tensor((thd + 180) % 360), "phi": torch.tensor(phd)}
    assert np.array_equal(digest(*G.get_masks(8, 8, 8, 16, cams)), ref["masks"])
    b = G.get_coords(16, 16, 16, 32, cams)
    assert np.array_equal(digest(*b), ref["coords"])
    for n in (16, 80, 160, 320):
        fb = G.spherical_freq_bands(n)
        assert np.array_equal(digest(fb), ref["pe%d_freq" % n]), n
        # (a seeded sample of the PE: sin / cos of float32 arguments up to 2^63 differ by one ulp between host CPUs)
        assert_within_one_ulp(G.spherical_pe(b[0], fb).reshape(-1)[ref["pe%d_idx" % n]].numpy(), ref["pe%d_val" % n])


# ---- the same operators off the benchmark grid: tests/golden/geometry_cameras.npz (tools/make_golden_geometry.py) holds the
# reference's answers for 34 cameras of any field of view, yaw and pitch (poles, seam, yaw outside one turn), non-square views
E2P_SIZES = ((16, 32, 16, 16), (32, 64, 12, 20), (17, 33, 9, 7), (64, 128, 32, 32))        # (eh, ew, h, w)
P2E_SIZES = ((16, 16, 16, 32), (12, 20, 32, 64), (9, 7, 17, 33))                           # (ph, pw, H, W)
MASK_SETS = (("cams5", (8, 8, 8, 16)), ("cams5", (6, 10, 8, 16)), ("cams5", (4, 4, 4, 8)), ("first13", (4, 4, 4, 8)))


@pytest.fixture(scope="module")
def geo():
    return golden("geometry_cameras.npz")


def _camera_dict(c):
    return {"FoV": torch.tensor(c[:, 0]), "theta": torch.tensor(c[:, 1]), "phi": torch.tensor(c[:, 2])}


def test_camera_list_of_the_geometry_fixture(geo):
    c = geo["cams"]
    assert c.shape == (34, 3) and c.dtype == np.float64
    assert 35 <= c[:24, 0].min() and c[:24, 0].max() <= 130 and c[:24, 1].min() < 0 and c[:24, 1].max() > 360
    assert [tuple(r) for r in c[24:29]] == [(90, 0, 0), (90, 0, 90), (90, 0, -90), (90, 180, 0), (90, 360, 0)]
    assert [tuple(r) for r in c[29:]] == [(90, -180, 45), (120, 359.999, 89.9), (60, 360 / 7, 0), (150, 12.5, -30), (20, 270, 10)]
    assert np.array_equal(geo["cams5"].T, [[90, 70, 110, 90, 60], [0, 33.3, 200, -45, 123.4], [0, 90, -60, 20, -89]])


@pytest.mark.parametrize("size", E2P_SIZES)
def test_e2p_grids_bit_exact_off_benchmark_cameras(geo, size):
    eh, ew, h, w = size
    maps = [G.e2p_grid(eh, ew, f, t, p, h, w) for f, t, p in geo["cams"]]
    bad = [i for i, m in enumerate(maps) if not np.array_equal(digest(*m), geo["e2p_grid_%dx%d_%dx%d" % size][i])]
    assert not bad, "cameras %s differ from the reference at %s" % (bad, size)
    if size == (17, 33, 9, 7):
        assert np.array_equal(np.stack([np.stack(m) for m in maps]), geo["e2p_maps_17x33_9x7"])


@pytest.mark.parametrize("size", P2E_SIZES)
def test_p2e_grids_and_masks_bit_exact_off_benchmark_cameras(geo, size):
    ph, pw, H, W = size
    key = "%dx%d_%dx%d" % size
    maps = [G.p2e_grid(ph, pw, f, t, p, H, W) for f, t, p in geo["cams"]]
    want_mask = np.unpackbits(geo["p2e_mask_" + key])[:34 * H * W].reshape(34, H, W).astype(bool)
    assert np.array_equal(np.stack([m[2] for m in maps]), want_mask)
    bad = [i for i, m in enumerate(maps) if not np.array_equal(digest(*m), geo["p2e_grid_" + key][i])]
    assert not bad, "cameras %s differ from the reference at %s" % (bad, size)
    if size == (9, 7, 17, 33):
        assert np.array_equal(np.stack([np.stack(m[:2]) for m in maps]), geo["p2e_maps_9x7_17x33"])


def test_remap_off_benchmark_cameras_non_square_view(geo):
    """e2p.py:54-76 / p2e.py:52-71 with one camera per sample: a 32x64 panorama and 12x20 views (hfov = h / w * fov)."""
    rng = np.random.default_rng(8)
    pano = torch.from_numpy(rng.standard_normal((34, 3, 32, 64)).astype(np.float32))
    views = torch.from_numpy(rng.standard_normal((34, 3, 12, 20)).astype(np.float32))
    cams = [torch.tensor(geo["cams"][:, k]) for k in range(3)]
    for mode in ("nearest", "bilinear"):
        assert np.array_equal(digest(G.e2p(pano, *cams, (12, 20), mode=mode)), geo["remap_e2p_" + mode]), mode
        assert np.array_equal(digest(*G.p2e(views, *cams, (32, 64), mode=mode)), geo["remap_p2e_" + mode]), mode


@pytest.mark.parametrize("which,shape", MASK_SETS)
def test_masks_off_benchmark_cameras(geo, which, shape):
    """models/pano/utils.py:10-84 with P = 16 and P = 60 (m * P no multiple of 32), pole cameras, m = 13."""
    c = geo["cams5"] if which == "cams5" else geo["cams"][:13]
    name = "%s_%dx%d_%dx%d" % ((which,) + shape)
    pers, equi = G.get_masks(*shape, _camera_dict(c))
    assert np.array_equal(digest(pers, equi), geo["masks_%s_digest" % name])
    assert np.array_equal(pers.numpy(), geo["masks_%s_pers" % name]) and np.array_equal(equi.numpy(), geo["masks_%s_equi" % name])


def test_coords_off_benchmark_cameras(geo):
    pers, equi = G.get_coords(12, 20, 16, 32, _camera_dict(geo["cams"]))
    assert np.array_equal(digest(pers, equi), geo["coords_digest"])
    assert np.array_equal(pers.numpy(), geo["coords_pers"]) and np.array_equal(equi.numpy(), geo["coords_equi"])


def test_pad_unpad(ref):
    g = torch.Generator().manual_seed(32)
    xs = (torch.randn(2, 3, 5, 16, generator=g), torch.randn(2, 2, 3, 5, 16, generator=g))
    for x, want, roundtrip in zip(xs, ref["pad2"], ref["unpad_roundtrip"]):
        assert np.array_equal(digest(G.pad_pano(x, 2)), want)
        assert bool(roundtrip) and torch.equal(G.unpad_pano(G.pad_pano(x, 3), 3), x)


def test_warpattn_matches_and_is_identity_at_init(ref):
    g = torch.Generator().manual_seed(33)
    px, ex = torch.randn(4, 64, 8, 8, generator=g), torch.randn(1, 64, 8, 16, generator=g)
    blk = MV.EPABlock(64)
    with torch.no_grad():
        po, eo = blk(px, ex, cam4())
    assert bool(ref["warpattn_identity_at_init"])                  # zero-init projections, in the reference ...
    assert torch.equal(po, px) and torch.equal(eo, ex)             # ... and in the port
    U.init_synthetic(blk, 3)
    MV.randomize_epa(blk, 4)
    sd = blk.state_dict()
    assert ["%s %s" % (k, tuple(v.shape)) for k, v in sd.items()] == list(ref["warpattn_keys"])
    assert np.array_equal(digest(*sd.values()), ref["warpattn_weights"])
    with torch.no_grad():
        b = blk(px, ex, cam4())
    assert rel_l2(b[0], torch.from_numpy(ref["warpattn_pers_out"])) < 1e-5
    assert rel_l2(b[1], torch.from_numpy(ref["warpattn_equi_out"])) < 1e-5


def test_denoiser_matches(ref):
    cfg = U.tiny_config(width=32, cross_attention_dim=64, heads=(1, 2, 4, 4), groups=8)
    unet, pano_unet = U.UNet2DConditionModel(**cfg), U.UNet2DConditionModel(**cfg)
    unet.add_lora(4)
    U.init_synthetic(unet, 1)
    U.init_synthetic(pano_unet, 2)
    torch.manual_seed(35)                      # the EPA weights that randomize_epa leaves at their default initialisation
    om = MV.DualBranchDenoiser(unet, pano_unet, None, None, True)
    MV.randomize_epa(om, 5)
    g = torch.Generator().manual_seed(34)
    b, m = 2, 4
    lat, pl = torch.randn(b, m, 4, 16, 16, generator=g), torch.randn(b, 1, 4, 16, 32, generator=g)
    t = torch.full((b, m), 981)
    pe, ppe = torch.randn(b, m, 7, 64, generator=g), torch.randn(b, 1, 7, 64, generator=g)
    cams = {k: torch.stack([v, v]) for k, v in cam4().items()}
    with torch.no_grad():
        o = om(lat, pl, t, pe, ppe, cams)
    assert rel_l2(o[0], torch.from_numpy(ref["denoiser_sample"])) < 1e-5
    assert rel_l2(o[1], torch.from_numpy(ref["denoiser_pano_sample"])) < 1e-5
    # rotation is NOT a roll of the geometry: different tables per offset
    c0 = {k: v.flatten() for k, v in cams.items()}
    c90 = dict(c0, theta=(c0["theta"] + 90) % 360)
    m0, m90 = G.get_masks(8, 8, 8, 16, c0)[0], G.get_masks(8, 8, 8, 16, c90)[0]
    assert not torch.equal(torch.roll(m0, 4, dims=2), m90)


def test_denoiser_matches_at_full_width_cfg1_first_call():
    """The port against the REFERENCE CLASS ITSELF at SD-2-base widths: BASELINE.json configs[0]'s first
    denoiser call of the loop -- m = 4 views of 32x32 latents + the 64x128 panorama latent, the CFG pair, t = 981, cameras and
    panorama rotated by the loop's first 90 degrees, weights / inputs from oracle/fixtures.py seeds.  tests/golden/ref_cfg1_call.npz
    holds what ``models.pano.MVGenModel.MultiViewBaseModel`` (models/pano/MVGenModel.py:38-297 with its WarpAttn / get_masks /
    SphericalPE / xformers-shimmed CrossAttention) returned around the same UNet objects as ``oracle.mvgen.DualBranchDenoiser``;
    both epsilon outputs agree to fp32 round-off (measured 2.6e-6).
    The same reference object drives tests/golden/cfg1_ddim10.npz (tools/make_golden_cfg.py cfg1)."""
    from oracle import fixtures as FX
    om = FX.build_full_width()
    a = golden("ref_cfg1_call.npz")
    args = FX.first_step_call(FX.horizon4_cameras(), (32, 32), (64, 128), cfg_pair=True)
    with torch.no_grad(), FX.chunked_attention():
        o = om(args["latents"], args["pano_latent"], args["timestep"], args["prompt_embd"], args["pano_prompt_embd"], args["cameras"])
    assert a["sample"].shape == (2, 4, 4, 32, 32) and a["pano_sample"].shape == (2, 1, 4, 64, 128)
    ev, ep = rel_l2(o[0], torch.from_numpy(a["sample"])), rel_l2(o[1], torch.from_numpy(a["pano_sample"]))
    print("\nport vs reference class at SD-2-base widths (cfg 1 first call): views %.2e  pano %.2e" % (ev, ep))
    assert ev < 1e-5 and ep < 1e-5, (ev, ep)


def test_py360_e2p_bit_exact(ref):
    """oracle/py360.py (numpy restatement incl. scipy's map_coordinates 'wrap' semantics) against the reference's own
    external/py360convert running on scipy: random cameras, odd sizes, uint8 / float32 / 2-D, both modes, an
    in-plane rotation, asymmetric field of view."""
    from oracle import py360
    rng = np.random.default_rng(11)
    k = 0
    for trial in range(12):
        H = int(rng.integers(9, 40))
        W = 2 * H + int(rng.integers(0, 3))
        img = (rng.random((H, W, 3)) * 255).astype(np.uint8) if trial % 3 == 0 else \
            rng.standard_normal((H, W, 2)).astype(np.float32) if trial % 3 == 1 else rng.standard_normal((H, W)).astype(np.float32)
        u, v = float(rng.uniform(-180, 180)), float(rng.uniform(-90, 90))
        fov = (float(rng.uniform(40, 120)), float(rng.uniform(40, 120)))
        hw = (int(rng.integers(5, 30)), int(rng.integers(5, 30)))
        rot = float(rng.uniform(-30, 30)) if trial % 4 == 0 else 0
        for mode in ("bilinear", "nearest"):
            got = py360.e2p(img, fov, u, v, hw, in_rot_deg=rot, mode=mode)
            assert got.dtype.str == ref["py360_e2p_dtype"][k] and np.array_equal(digest(got), ref["py360_e2p"][k]), (trial, mode)
            k += 1
    assert k == len(ref["py360_e2p"])
