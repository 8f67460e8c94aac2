"""mp2e without a GPU: the float64 model (tests/mp2e_model.py) against the reference fixture tests/golden/mp2e.npz
(tools/make_golden_mp2e.py: the reference's own tensor p2e), properties of the model, host-side argument validation of
pf_mp2e (every case fails before any launch) and the ValueErrors of the Python forms."""
import ctypes as C

import numpy as np
import pytest
import torch

import mp2e_model as M
from conftest import golden
from panfusion_amd import _lib


@pytest.fixture(scope="module")
def gd():
    return golden("mp2e.npz")


def _inputs(gd, case):
    return tuple(gd[case + "_" + k].astype(np.float64) for k in ("imgs", "fov", "theta", "phi"))


@pytest.mark.parametrize("case,mode,feather", M.keys())
def test_model_reproduces_the_reference_fixture(gd, case, mode, feather):
    """Float64 result within 1e-9 absolute (float64 rounding on the 0-255 scale) and the same uncovered set, exactly."""
    imgs, fov, theta, phi = _inputs(gd, case)
    k = M.key(case, mode, feather)
    assert imgs.shape[:3] == (M.CASES[case]["B"], fov.shape[1], M.CASES[case]["C"])
    for b in range(imgs.shape[0]):
        out, den = M.mp2e(imgs[b], fov[b], theta[b], phi[b], M.CASES[case]["pano"], mode, feather)
        assert np.array_equal(den == 0, gd[k + "_wsum"][b] == 0)
        assert np.abs(out - gd[k + "_out"][b]).max() <= 1e-9
        assert np.abs(den - gd[k + "_wsum"][b]).max() <= 1e-12


def test_fixture_covers_the_arms_it_is_there_for(gd):
    assert gd["ico_fov"].shape == (1, 20) and gd["hor_fov"].shape == (2, 8) and not np.array_equal(gd["hor_theta"][0], gd["hor_theta"][1])
    assert float((gd["ico_bilinear_horizontal_wsum"] == 0).mean()) == 0.0                    # full coverage
    assert float((gd["hor_bilinear_horizontal_wsum"] == 0).mean()) >= 0.4                    # the fill arm
    w = gd["rnd_bilinear_both_wsum"]
    assert 0 < w[w > 0].min() < 1e-3                                                          # small total weights
    assert len(set(np.round(gd["rnd_fov"][0], 6))) == 5                                       # per-view FoV
    for case, mode, feather in M.keys():
        assert 0 <= float(gd[M.key(case, mode, feather) + "_e32"]) < 1e-3


def test_tent_follows_numpy_linspace():
    assert np.array_equal(M.tent(2), [0.0, 1.0])                                              # linspace(num=1) is [start]
    assert np.array_equal(M.tent(8), np.concatenate([np.linspace(0, 1, 4), np.linspace(1, 0, 4)]))
    with pytest.raises(ValueError):
        M.tent(7)
    both = M.tent_image(4, 6, "both", np.float32)
    assert both.dtype == np.float32 and np.array_equal(both, M.tent(4).astype(np.float32)[:, None] * M.tent(6).astype(np.float32)[None])


@pytest.mark.parametrize("mode", M.MODES)
def test_model_properties(gd, mode):
    imgs, fov, theta, phi = (a[0] for a in _inputs(gd, "rnd"))
    from oracle import geometry as G
    (h, w), hw = M.CASES["rnd"]["view"], M.CASES["rnd"]["pano"]
    for feather in ("horizontal", "both"):
        out, den = M.mp2e(imgs, fov, theta, phi, hw, mode, feather)
        seen = den > 0
        assert 0 < seen.mean() < 1
        # Where a contributing view is sampled below its last row (v in (h - 1, h]) with bilinear taps and the column tent
        # alone, the zero padding of the tensor p2e enters the image sample and the tent sample alike: (1 - wy) twice in
        # the numerator, once in the denominator, and the pixel is darkened.  (Feather both has weight 0 there; a nearest
        # tap outside the view contributes nothing.)
        below = np.zeros(hw, bool)
        if mode == "bilinear" and feather == "horizontal":
            for i in range(len(fov)):
                _, v, mask = G.p2e_grid(h, w, fov[i], theta[i], phi[i], *hw)
                below |= mask & (M.position(v, h) > h - 1)
            assert (below & seen).any()
        clean = seen & ~below
        # within [min, max] of the inputs up to rounding (darkened pixels: [0, max]), or the fill value
        assert np.all(out[:, ~seen] == 255.0)
        assert out[:, clean].min() >= imgs.min() - 1e-9 and out[:, seen].min() >= 0.0 and out[:, seen].max() <= imgs.max() + 1e-9
        # a constant image stays constant wherever the weight is positive and no view is sampled below its last row
        flat, den_c = M.mp2e(np.full_like(imgs, 37.5), fov, theta, phi, hw, mode, feather)
        assert np.array_equal(den_c, den) and np.abs(flat[:, clean] - 37.5).max() <= 1e-11
        assert not (below & seen).any() or flat[:, below & seen].min() < 36.5
        # the order of the views changes nothing beyond rounding
        perm = np.array([3, 0, 4, 2, 1])
        out_p, den_p = M.mp2e(imgs[perm], fov[perm], theta[perm], phi[perm], hw, mode, feather)
        assert np.array_equal(den_p == 0, den == 0)
        assert np.abs(den_p - den).max() <= 1e-12 and np.abs(out_p - out)[:, seen].max() <= 1e-9 * max(1.0, 1.0 / den[seen].min())


@pytest.mark.parametrize("mode", M.MODES)
def test_single_view_weight_is_the_sampled_tent_times_the_mask(gd, mode):
    from oracle import geometry as G
    imgs, fov, theta, phi = (a[0] for a in _inputs(gd, "one"))
    (h, w), hw = M.CASES["one"]["view"], M.CASES["one"]["pano"]
    _, den = M.mp2e(imgs, fov, theta, phi, hw, mode, "horizontal")
    u, v, mask = G.p2e_grid(h, w, 75.0, 30.0, 20.0, *hw)
    want = M.sample(M.tent_image(h, w, "horizontal")[None], u, v, mode)[0] * mask
    assert np.array_equal(den, want) and mask.any() and not mask.all()
    if mode == "bilinear":
        # the SAMPLE of the tent image, not the two ramps evaluated at the position: between the two centre columns both
        # taps are 1 and the sample is flat, where the extended ramp min(x, w - 1 - x) / (w / 2 - 1) exceeds 1
        px, py = M.position(u, w), M.position(v, h)
        across = mask & (px > w // 2 - 1) & (px < w // 2) & (py >= 0) & (py <= h - 1)
        assert across.any() and np.abs(den[across] - 1.0).max() <= 1e-12
        assert (np.minimum(px, w - 1 - px)[across] / (w // 2 - 1)).min() > 1.0


# ------------------------------------------------------------------------------------------------ C entry, host side
def _call(**kw):
    """pf_mp2e on fake (never dereferenced) device addresses: structurally valid, kw overrides."""
    a = dict(src=0x10000, dtype=_lib.PF_F32, B=2, m=3, C=3, ph=8, pw=8, cam_batch=2, H=16, W=32, mode=1, feather=0, fill=255.0,
             out=0x20000, weight=0x30000, ws=0x40000, ws_bytes=None, fov=[90.0] * 6)
    a.update(kw)
    lib = _lib.lib()
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.pf_mp2e_workspace_size(a["B"], a["m"])
    arr = lambda v: (C.c_double * len(v))(*v)
    n = len(a["fov"])
    return lib.pf_mp2e(a["src"], a["dtype"], a["B"], a["m"], a["C"], a["ph"], a["pw"], arr(a["fov"]), arr([10.0] * n), arr([5.0] * n),
                       a["cam_batch"], a["H"], a["W"], a["mode"], a["feather"], a["fill"], a["out"], a["weight"], a["ws"],
                       a["ws_bytes"], None)


def test_pf_mp2e_rejects_bad_arguments_before_any_launch():
    lib = _lib.lib()
    need = lib.pf_mp2e_workspace_size(2, 3)
    bad = [
        (dict(pw=7), b"must be even"),
        (dict(ph=7, feather=1), b"height 7 must be even"),
        (dict(mode=2), b"mode"),
        (dict(feather=2), b"feather"),
        (dict(ws_bytes=need - 1), b"workspace too small"),
        (dict(out=None), b"null pointer"),
        (dict(src=None), b"null pointer"),
        (dict(ws=None), b"null pointer"),
        (dict(cam_batch=3), b"cam_batch"),
        (dict(dtype=_lib.PF_U8), b"dtype"),
        (dict(H=1), b"sizes must be > 1"),
        (dict(ph=1), b"sizes must be > 1"),
        (dict(C=0), b"bad sizes"),
        (dict(fill=float("inf")), b"fill"),
        (dict(fill=float("nan")), b"fill"),
        (dict(fov=[90.0, 180.0] * 3), b"fov[1]"),
    ]
    for kw, needle in bad:
        assert _call(**kw) == 1, kw
        assert needle in lib.pf_last_error_string(), (kw, lib.pf_last_error_string())
    assert _call(ph=7, feather=0, mode=99) == 1 and b"mode" in lib.pf_last_error_string()      # odd height is legal without feather both


def test_workspace_size_is_host_arithmetic():
    lib = _lib.lib()
    one = lib.pf_mp2e_workspace_size(1, 1)
    assert one > 0 and one % 256 == 0
    assert lib.pf_mp2e_workspace_size(1, 20) >= 20 * 38 * 8 and lib.pf_mp2e_workspace_size(2, 20) >= 40 * 38 * 8
    assert lib.pf_mp2e_workspace_size(4, 5) == lib.pf_mp2e_workspace_size(5, 4) == lib.pf_mp2e_workspace_size(1, 20)
    assert lib.pf_mp2e_workspace_size(0, 3) == 0


# ------------------------------------------------------------------------------------------------ Python forms
def test_mp2e_value_errors():
    from panfusion_amd.external.Perspective_and_Equirectangular import mp2e
    cam = ([90.0] * 3, [0.0, 10.0, 20.0], [0.0] * 3)
    with pytest.raises(ValueError, match="views must be"):
        mp2e(torch.zeros(3, 8, 8), *cam, (16, 32))
    with pytest.raises(ValueError, match="views must be"):
        mp2e(np.zeros((1, 3, 8, 8, 3)), *cam, (16, 32))
    with pytest.raises(ValueError, match="even"):
        mp2e(torch.zeros(3, 3, 8, 7), *cam, (16, 32))
    with pytest.raises(ValueError, match="even"):
        mp2e(torch.zeros(3, 3, 7, 8), *cam, (16, 32), feather="both")
    with pytest.raises(ValueError, match="even"):
        mp2e(np.zeros((3, 8, 7, 3), np.uint8), *cam, (16, 32))
    with pytest.raises(ValueError, match="cameras"):
        mp2e(torch.zeros(4, 3, 8, 8), *cam, (16, 32))
    with pytest.raises(ValueError, match="cameras"):
        mp2e(torch.zeros(3, 3, 8, 8), [90.0] * 3, [0.0] * 2, [0.0] * 3, (16, 32))
    with pytest.raises(ValueError, match="cameras"):
        mp2e(torch.zeros(2, 3, 3, 8, 8), [90.0] * 4, [0.0] * 4, [0.0] * 4, (16, 32))
    with pytest.raises(ValueError, match="feather"):
        mp2e(torch.zeros(3, 3, 8, 8), *cam, (16, 32), feather="vertical")
    with pytest.raises(ValueError, match="mode"):
        mp2e(torch.zeros(3, 3, 8, 8), *cam, (16, 32), mode="bicubic")
    with pytest.raises(TypeError):
        mp2e([[1.0]], *cam, (16, 32))


def test_stitch_views_and_from_views_value_errors():
    from panfusion_amd.pipeline import KnownRegion, stitch_views
    cams = {"FoV": torch.full((1, 3), 90.0), "theta": torch.tensor([[0.0, 10.0, 20.0]]), "phi": torch.zeros(1, 3)}
    with pytest.raises(ValueError, match="stitch_views"):
        stitch_views(torch.zeros(3, 8, 8, 3, dtype=torch.uint8), cams, (16, 32))
    with pytest.raises(ValueError, match="cameras"):
        stitch_views(torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8), cams, (16, 32))
    with pytest.raises(ValueError, match="cameras"):
        stitch_views(torch.zeros(1, 3, 3, 8, 8), dict(cams, phi=torch.zeros(3)), (16, 32))
    with pytest.raises(ValueError, match="from_views"):
        KnownRegion.from_views(None, torch.zeros(1, 2, 3, 8, 8), [90.0], [0.0], [0.0], cams, (2, 4), (1, 1))
    with pytest.raises(ValueError, match="from_views"):
        KnownRegion.from_views(None, torch.zeros(2, 4, 8, 8), [90.0] * 2, [0.0] * 2, [0.0] * 2, cams, (2, 4), (1, 1))
    with pytest.raises(ValueError, match="cameras"):
        KnownRegion.from_views(None, torch.zeros(2, 3, 8, 8), [90.0] * 2, [0.0] * 3, [0.0] * 2, cams, (2, 4), (1, 1))
