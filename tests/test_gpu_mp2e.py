"""pf_mp2e on the GPU: against the reference fixture tests/golden/mp2e.npz (tools/make_golden_mp2e.py), against the same sum
composed from pf_p2e_grid + pf_remap (pins the addressing), dtype / batch / camera-sharing / repeatability identities, the
numpy form, stitch_views and KnownRegion.from_views."""
import numpy as np
import pytest
import torch

import mp2e_model as M
from conftest import build_tiny_oracle, cam4, golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def gd():
    return golden("mp2e.npz")


def _case(gd, case):
    """views (B, m, C, h, w) fp32 on the GPU, cameras as three flat (B * m) float64 arrays."""
    cams = tuple(gd[case + "_" + k].reshape(-1) for k in ("fov", "theta", "phi"))
    return torch.from_numpy(gd[case + "_imgs"]).to(DEV), cams


def _run(src, cams, case, mode, feather="horizontal", **kw):
    from panfusion_amd import ops
    return ops.mp2e(src, *cams, M.CASES[case]["pano"], mode, feather, want_weight=True, **kw)


def _ulps(a, b):
    a, b = (t.contiguous().view(torch.int32).long() for t in (a, b))
    return (a - b).abs()


@pytest.mark.parametrize("case,mode,feather", M.keys())
def test_against_the_reference_fixture(gd, case, mode, feather):
    """The uncovered set equals the fixture's exactly.  Elsewhere max |out - out64| <= 4 e32, e32 = what the reference's own
    float32 composition loses against its float64 one on the same input (the kernel sums in one fixed order and forms bilinear
    weights as 1 - f, each a few ulp from torch's forms; a wrong tap, camera, tent index or mask costs whole grey levels).
    The summed weight is held the same way on its own scale: max |weight - wsum64| <= 4 e32_w, e32_w the same float32-against-
    float64 loss measured on the reference's summed weight.  Ratios to the bound are printed with -s."""
    src, cams = _case(gd, case)
    out, weight = _run(src, cams, case, mode, feather)
    k = M.key(case, mode, feather)
    out64, w64 = torch.from_numpy(gd[k + "_out"]), torch.from_numpy(gd[k + "_wsum"])
    e32, e32_w = float(gd[k + "_e32"]), float(gd[k + "_e32_w"])
    assert out.dtype == weight.dtype == torch.float32 and out.shape == out64.shape and weight.shape == (out.shape[0], 1) + out.shape[2:]
    weight = weight[:, 0].cpu().double()
    zero = w64 == 0
    assert torch.equal(weight == 0, zero)
    out = out.cpu().double()
    assert bool((out[zero[:, None].expand_as(out)] == 255.0).all())
    err = float(((out - out64).abs() * (~zero)[:, None]).max())
    err_w = float((weight - w64).abs().max())
    print("\n%s: out err %.3e (%.2f of 4 e32 = %.3e), weight err %.3e (%.2f of 4 e32_w = %.3e)"
          % (k, err, err / (4 * e32) if e32 else 0.0, 4 * e32, err_w, err_w / (4 * e32_w) if e32_w else 0.0, 4 * e32_w))
    assert err <= 4 * e32, (err, e32)
    assert err_w <= 4 * e32_w, (err_w, e32_w)


@pytest.mark.parametrize("case", ["ico", "rnd"])
@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("feather", ["horizontal", "both"])
def test_against_the_composition_from_existing_entry_points(gd, case, mode, feather):
    """sum_i remap(img_i) remap(tent_i) and sum_i remap(tent_i) from pf_p2e_grid + pf_remap, added in camera order in float32 on the
    GPU: the kernel's terms are the same floats, so the weight is bit-identical and out agrees within 2 ulp (the one division)."""
    from panfusion_amd import ops
    src, cams = _case(gd, case)
    (h, w), (H, W) = M.CASES[case]["view"], M.CASES[case]["pano"]
    out, weight = _run(src, cams, case, mode, feather)
    mu, mv, mask = ops.p2e_grid(*cams, h, w, H, W, DEV)
    tent = torch.from_numpy(M.tent_image(h, w, feather, np.float32)).to(DEV)[None, None]
    num = torch.zeros(src.shape[2], H, W, device=DEV)
    den = torch.zeros(H, W, device=DEV)
    for i in range(src.shape[1]):
        maps = (mu[i:i + 1], mv[i:i + 1], mode)
        term = ops.remap(src[0, i:i + 1], *maps, mask=mask[i:i + 1])[0]
        wgt = ops.remap(tent, *maps, mask=mask[i:i + 1])[0, 0]
        prod = term * wgt
        num = num + prod
        den = den + wgt
    assert torch.equal(weight[0, 0], den)
    seen = den > 0
    assert 0 < int(seen.sum())
    ulps = _ulps(out[0], num / torch.where(seen, den, torch.ones_like(den)))[:, seen]
    print("\n%s %s %s: %d of %d elements differ, at most %d ulp" % (case, mode, feather, int((ulps > 0).sum()), ulps.numel(), int(ulps.max())))
    assert int(ulps.max()) <= 2
    assert bool((out[0][:, ~seen] == 255.0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mode", M.MODES)
def test_16_bit_sources_equal_the_fp32_kernel_on_the_upcast(gd, dtype, mode):
    src, cams = _case(gd, "rnd")
    low = src.to(dtype)
    a, wa = _run(low, cams, "rnd", mode, "both")
    b, wb = _run(low.float(), cams, "rnd", mode, "both")
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(wa, wb)
    assert not torch.equal(a, _run(src, cams, "rnd", mode, "both")[0])


@pytest.mark.parametrize("mode", M.MODES)
def test_batches_cameras_and_repeats(gd, mode):
    """B = 2 with per-batch cameras equals two B = 1 calls; cameras shared by the batch equal the same cameras repeated; a second
    call is bit-identical; fill is a parameter.  All bit for bit."""
    src, cams = _case(gd, "hor")
    m = src.shape[1]
    out, weight = _run(src, cams, "hor", mode)
    for b in range(2):
        ob, wb = _run(src[b:b + 1], tuple(c[b * m:(b + 1) * m] for c in cams), "hor", mode)
        assert torch.equal(out[b:b + 1], ob) and torch.equal(weight[b:b + 1], wb)
    assert not torch.equal(weight[0], weight[1])
    first = tuple(c[:m] for c in cams)
    shared, ws_ = _run(src, first, "hor", mode)
    repeated, wr = _run(src, tuple(np.concatenate([c, c]) for c in first), "hor", mode)
    assert torch.equal(shared, repeated) and torch.equal(ws_, wr) and torch.equal(shared[0], out[0]) and not torch.equal(shared[1], out[1])
    again, wa = _run(src, cams, "hor", mode)
    assert torch.equal(again, out) and torch.equal(wa, weight)
    other, wo = _run(src, cams, "hor", mode, fill=-3.5)
    hole = (weight == 0).expand_as(out)
    assert torch.equal(wo, weight) and bool((other[hole] == -3.5).all()) and torch.equal(other[~hole], out[~hole]) and int(hole.sum()) > 0


@pytest.mark.parametrize("case", ["ico", "hor", "w2"])
@pytest.mark.parametrize("mode", M.MODES)
def test_numpy_form(gd, case, mode):
    """The reference's own calling form: (m, h, w, 3) numpy in, uint8 (H, W, 3) out by truncation; 255 on the fixture's uncovered
    set, every element within 1 grey level of trunc of the fixture's float64 result (the float bound is far below 1, and
    truncation moves a value that sits on an integer by one level: no element is exempt)."""
    from panfusion_amd.external.Perspective_and_Equirectangular import mp2e
    views = np.ascontiguousarray(gd[case + "_imgs"][0].transpose(0, 2, 3, 1))
    cams = tuple(gd[case + "_" + k][0] for k in ("fov", "theta", "phi"))
    H, W = M.CASES[case]["pano"]
    got = mp2e(views, *cams, (H, W), mode)
    k = M.key(case, mode, "horizontal")
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (H, W, 3)
    zero = gd[k + "_wsum"][0] == 0
    assert np.all(got[zero] == 255)
    want = gd[k + "_out"][0].transpose(1, 2, 0).astype(np.uint8)
    assert int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()) <= 1
    got2, w = mp2e(views, *cams, (H, W), mode, return_weight=True)
    assert np.array_equal(got2, got) and w.shape == (H, W) and np.array_equal(w == 0, zero)


def test_tensor_form_and_stitch_views(gd):
    from panfusion_amd.external.Perspective_and_Equirectangular import mp2e
    from panfusion_amd.pipeline import stitch_views
    src, cams = _case(gd, "ico")
    want, wsum = _run(src, cams, "ico", "bilinear")
    got = mp2e(src[0], *cams, M.CASES["ico"]["pano"])
    assert got.shape == want.shape[1:] and torch.equal(got, want[0])
    got5, w5 = mp2e(src, *cams, M.CASES["ico"]["pano"], return_weight=True)
    assert torch.equal(got5, want) and torch.equal(w5, wsum)
    cam = {k: torch.from_numpy(gd["ico_" + n]) for k, n in (("FoV", "fov"), ("theta", "theta"), ("phi", "phi"))}
    u8 = src.permute(0, 1, 3, 4, 2).to(torch.uint8).contiguous()                 # (1, m, h, w, 3), as decode_views_and_pano returns
    pano = stitch_views(u8, cam, M.CASES["ico"]["pano"], feather="both")
    assert pano.shape == want.shape and torch.equal(pano, _run(u8.permute(0, 1, 4, 2, 3).float(), cams, "ico", "bilinear", "both")[0])
    assert torch.equal(stitch_views(src, cam, M.CASES["ico"]["pano"]), want)


# --------------------------------------------------------------------------------------------------------- outpainting
@pytest.fixture(scope="module")
def tiny_encoder():
    from oracle import sd2_unet as U
    from oracle import vae as OV
    from panfusion_amd import vae as PV
    from panfusion_amd.models.vae_params import VAEEncoderParams
    cfg = OV.tiny_vae_config(width=64, groups=8)
    ov = OV.AutoencoderKLDecoder(**cfg)
    U.init_synthetic(ov, 81)
    enc = VAEEncoderParams(**cfg)
    enc.load_state_dict({k: v for k, v in ov.state_dict().items() if k.startswith(("encoder.", "quant_conv."))}, strict=True)
    return PV.VAEEncoder(enc, compute_dtype=torch.float16)


def test_from_views_is_mp2e_then_from_panorama_and_the_loop_keeps_it(tiny_encoder):
    """Three overlapping photos -> KnownRegion.from_views: the panorama mask is the 8x8 block rule on weight == 0 of a direct mp2e
    call, every tensor equals from_panorama on that stitched panorama bit for bit, and a two-step DenoiseLoop at the tiny widths
    returns the kept latent pixels exactly."""
    from panfusion_amd.external.Perspective_and_Equirectangular import mp2e
    from panfusion_amd.models.pano import MultiViewBaseModel
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion
    g = golden("mvgen_tiny.npz")
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    lat, pano, pe, ppe = t("latents")[:1], t("pano_latent")[:1], t("prompt_embd"), t("pano_prompt_embd")
    cams = {k: v[None] for k, v in cam4().items()}
    pano_hw, view_hw = tuple(pano.shape[-2:]), tuple(lat.shape[-2:])
    photos = (torch.rand(3, 3, 48, 64, generator=torch.Generator().manual_seed(15)) * 2 - 1).to(DEV)
    shot = ([80.0, 90.0, 70.0], [-20.0, 30.0, 35.0], [5.0, 0.0, 40.0])
    known = KnownRegion.from_views(tiny_encoder, photos, *shot, cams, pano_hw, view_hw)
    stitched, weight = mp2e(photos, *shot, (8 * pano_hw[0], 8 * pano_hw[1]), "bilinear", feather="both", fill=0.0, return_weight=True)
    gen = (weight == 0).float()
    assert torch.equal(known.pano_mask[0], torch.nn.functional.max_pool2d(gen[None], 8))
    assert 0 < float(known.pano_mask.mean()) < 1 and bool((stitched[:, weight[0] == 0] == 0).all())
    want = KnownRegion.from_panorama(tiny_encoder, stitched[None, None], gen[None, None], cams, view_hw)
    for a, b in ((known.latents, want.latents), (known.mask, want.mask), (known.pano_latent, want.pano_latent), (known.pano_mask, want.pano_mask)):
        assert torch.equal(a, b)
    # one photo: the tent is 0 on the outermost columns and rows, so from_views keeps no more than from_view does
    single = KnownRegion.from_views(tiny_encoder, photos[:1], [80.0], [-20.0], [5.0], cams, pano_hw, view_hw)
    plain = KnownRegion.from_view(tiny_encoder, photos[:1], 80.0, -20.0, 5.0, cams, pano_hw, view_hw)
    assert bool((single.pano_mask >= plain.pano_mask).all()) and int((plain.pano_mask == 0).sum()) > 0

    om = build_tiny_oracle()
    model = MultiViewBaseModel(om.unet, om.pano_unet, None, None, om.pano_pad, compute_dtype=torch.float16)
    model.load_state_dict({k: v for k, v in om.state_dict().items() if k.startswith("cp_blocks")}, strict=False)
    out_lat, out_pano = DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=2, known=known).run()
    assert torch.isfinite(out_lat).all() and torch.isfinite(out_pano).all()
    keep_v, keep_p = (known.mask == 0).expand_as(out_lat), (known.pano_mask == 0).expand_as(out_pano)
    assert int(keep_v.sum()) > 0 and int(keep_p.sum()) > 0
    assert torch.equal(out_lat[keep_v], known.latents[keep_v].float()) and torch.equal(out_pano[keep_p], known.pano_latent[keep_p].float())
