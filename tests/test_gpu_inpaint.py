"""Known-region sampling (inpainting / outpainting) on the MI355X: pf_cfg_inpaint_step_pair against a float64 torch statement,
mask = 1 / mask = 0 against the plain update kernels and the known latent bit for bit, the cfg 1 trajectory against the fixture
tools/make_golden_inpaint.py wrote with the reference class as the denoiser (diffusers' form of the blend, operands rolled with
the state), graph replay against eager launches, the KnownRegion builders on the tiny VAE, and one short cfg 2 outpainting run.
Needs an MI355X: `-m gpu`."""
import pytest
import torch

from conftest import cam4, golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _masks(shape, seed):
    """A binary mask and a soft one (values in [0, 1], a quarter of them exactly 0 or 1), fp32, the shape of the latent."""
    g = torch.Generator().manual_seed(seed)
    binary = (torch.rand(shape, generator=g) < 0.5).float()
    soft = torch.rand(shape, generator=g)
    soft[..., ::4] = binary[..., ::4]
    return binary, soft


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape", [(1, 20, 4, 64, 64), (1, 1, 4, 64, 128), (1, 1, 4, 128, 256)])
def test_inpaint_step_pair_vs_float64(shape):
    """cfg 2's view and panorama latents and a 256-wide panorama; rolls 0, W/4, 17, -5 x known_roll 0, W/4, 13; the DDIM form
    and the 2M form; binary and soft masks; in place (out = x, x0_out = x0_prev) and out of place: out within 2e-6 rel-L2 of
    m v + (1 - m)(ka z + kb n) in float64 (fp32 coefficients, operands read at (w - known_roll) mod W, the result rolled),
    out2 == out bit for bit, the timestep words written, x0_out the 2M kernel's bit for bit."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DPMSolverSchedule
    sched = DPMSolverSchedule()
    sched.set_timesteps(50)
    W = shape[-1]
    x, eu, ec, hist = rnd(*shape, seed=41), rnd(*shape, seed=42), rnd(*shape, seed=43), rnd(*shape, seed=44) * 0.5
    z, n = rnd(*shape, seed=45), rnd(*shape, seed=46)
    d = lambda v: v.to(DEV)
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))
    for form in ("ddim", "2m"):
        for i, roll in ((1, 0), (20, W // 4), (37, 17), (48, -5)):
            coef, k, order = sched.step_coefficients(i)
            ka, kb = coef[2:]
            sa, sb, sap, sbp = (torch.tensor(c, dtype=torch.float32).double() for c in coef)
            eps = eu.double() + 9.0 * (ec.double() - eu.double())
            x0 = (x.double() - sb * eps) / sa
            v = sap * x0 + sbp * eps
            if form == "2m":
                v = v + f32(k) * (x0 - hist.double())
            t_next = sched.timesteps[i + 1]
            for kr in (0, W // 4, 13):
                for mi, mask in enumerate(_masks(shape, seed=i + kr)):
                    r = lambda t: torch.roll(t.double(), kr, -1)
                    want = torch.roll(r(mask) * v + (1 - r(mask)) * (f32(ka) * r(z) + f32(kb) * r(n)), roll, -1)
                    blend = dict(known=d(z), noise=d(n), mask=d(mask), ka=ka, kb=kb, known_roll=kr)
                    for in_place in (False, True):
                        pair = torch.stack([x[0], x[0]]).to(DEV)
                        h = d(hist)
                        tstep = torch.full((2, 5), 7, dtype=torch.long, device=DEV)
                        hx = dict(x0_prev=h, k=k, x0_out=h) if form == "2m" else {}
                        if in_place:
                            out, x0_out = ops.cfg_inpaint_step_pair(pair[:1], d(eu), d(ec), 9.0, coef, roll, out=pair[:1],
                                                                    out2=pair[1:], tstep=tstep, t_next=t_next, **hx, **blend)
                            assert out.data_ptr() == pair.data_ptr()
                            out2 = pair[1:]
                        else:
                            out2 = torch.empty_like(pair[1:])
                            if form == "2m":
                                hx["x0_out"] = torch.empty_like(h)
                            out, x0_out = ops.cfg_inpaint_step_pair(d(x), d(eu), d(ec), 9.0, coef, roll, out2=out2, tstep=tstep,
                                                                    t_next=t_next, **hx, **blend)
                        e = rel_l2(out.cpu(), want)
                        assert e <= 2e-6, (shape, form, i, roll, kr, mi, in_place, e)
                        assert torch.equal(out2, out)
                        assert torch.equal(tstep.cpu(), torch.full((2, 5), t_next, dtype=torch.long))
                        if form == "2m":
                            _, x0_ref = ops.cfg_dpmpp_step_pair(d(x), d(eu), d(ec), 9.0, coef, roll, x0_prev=d(hist), k=k)
                            assert torch.equal(x0_out, x0_ref)
                        else:
                            assert x0_out is None


@pytest.mark.parametrize("shape", [(1, 20, 4, 64, 64), (1, 1, 4, 64, 128)])
def test_mask_one_is_the_update_kernel_and_mask_zero_is_known(shape):
    """m = 1: pf_cfg_ddim_step_pair / pf_cfg_dpmpp_step_pair bit for bit (state and history).  m = 0 with (ka, kb) = (1, 0): the
    known latent read at the offset and rolled, bit for bit, whatever the update."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DPMSolverSchedule
    sched = DPMSolverSchedule()
    sched.set_timesteps(20)
    W = shape[-1]
    x, eu, ec, hist, z, n = (rnd(*shape, seed=51 + j).to(DEV) for j in range(6))
    ones, zeros = torch.ones_like(x), torch.zeros_like(x)
    for i, roll, kr in ((3, 0, 0), (7, W // 4, W // 4), (11, -5, 13), (18, 17, W - 1)):
        coef, k, _ = sched.step_coefficients(i)
        kw = dict(known=z, noise=n, ka=coef[2], kb=coef[3], known_roll=kr)
        got, _ = ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, roll, mask=ones, **kw)
        assert torch.equal(got, ops.cfg_ddim_step_pair(x, eu, ec, 9.0, coef, roll))
        got, got_x0 = ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, roll, x0_prev=hist, k=k, x0_out=torch.empty_like(x),
                                                mask=ones, **kw)
        want, want_x0 = ops.cfg_dpmpp_step_pair(x, eu, ec, 9.0, coef, roll, x0_prev=hist, k=k)
        assert torch.equal(got, want) and torch.equal(got_x0, want_x0)
        kept = torch.roll(torch.roll(z, kr, -1), roll, -1)
        kw.update(ka=1.0, kb=0.0)
        got, _ = ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, roll, mask=zeros, **kw)
        assert torch.equal(got, kept)
        got, _ = ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, roll, x0_prev=hist, k=k, x0_out=torch.empty_like(x), mask=zeros, **kw)
        assert torch.equal(got, kept)


def test_inpaint_step_pair_rejects_bad_arguments():
    from panfusion_amd import _lib, ops
    coef = (0.5, 0.8, 0.6, 0.7)
    x, eu, ec, h, z, n, m = (torch.zeros(1, 4, 8, 64, device=DEV) for _ in range(7))
    out = torch.empty_like(x)
    blend = dict(known=z, noise=n, mask=m, ka=0.6, kb=0.7, known_roll=5)
    wide = torch.zeros(1, 8193, device=DEV)
    wb = dict(known=wide.clone(), noise=wide.clone(), mask=wide.clone(), ka=0.6, kb=0.7)
    with pytest.raises(_lib.PanFusionHipError, match="8192"):
        ops.cfg_inpaint_step_pair(wide, wide.clone(), wide.clone(), 9.0, coef, x0_out=wide.clone(), **wb)
    wider = torch.zeros(1, 16385, device=DEV)
    wb = dict(known=wider.clone(), noise=wider.clone(), mask=wider.clone(), ka=0.6, kb=0.7)
    with pytest.raises(_lib.PanFusionHipError, match="16384"):
        ops.cfg_inpaint_step_pair(wider, wider.clone(), wider.clone(), 9.0, coef, **wb)
    bad = [dict(out=out, **dict(blend, known=None)), dict(out=out, **dict(blend, mask=None)),
           dict(out=out, **dict(blend, noise=out)), dict(out=out, **dict(blend, known=out)),
           dict(out=out, x0_out=h, **dict(blend, mask=h)), dict(out=out, x0_prev=h, **blend),
           dict(out=out, x0_out=out, **blend), dict(out=x, out2=x, **blend)]
    for kw in bad:
        with pytest.raises(_lib.PanFusionHipError):
            ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, 3, **kw)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def full_width():
    from oracle import fixtures as FX
    return FX.build_full_width()


def _hip_model(om):
    from panfusion_amd.models.pano import MultiViewBaseModel
    model = MultiViewBaseModel(om.unet, om.pano_unet, None, None, True, compute_dtype=torch.float16)      # default: fp16 mixed
    model.load_state_dict({k: v for k, v in om.state_dict().items() if k.startswith("cp_blocks")}, strict=False)
    assert model.precision == "mixed"
    return model


def _fixture_known(gd):
    from panfusion_amd.pipeline import KnownRegion
    t = lambda k: torch.from_numpy(gd[k]).to(DEV)
    return KnownRegion(t("known_latents"), t("known_mask"), t("known_pano"), t("known_pano_mask"))


def _cfg1_loop(model, graphs, known, sampler="ddim", steps=10):
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    return DenoiseLoop(model, latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=steps,
                       use_graphs=graphs, sampler=sampler, known=known)


def _trajectory(loop):
    """(views, panorama in the un-rotated frame) after every step, as DenoiseLoop.result un-rolls it."""
    from panfusion_amd import ops
    traj = []
    for _ in range(len(loop.timesteps)):
        loop.step()
        traj.append((loop.lat.clone(), ops.roll_width(loop.pano, int(-loop.total_rot / 360 * loop.W)).clone()))
    return traj


@pytest.mark.parametrize("graphs", [True, False])
def test_cfg1_ten_inpaint_steps_vs_oracle(full_width, graphs):
    """BASELINE.json configs[0] (m = 4 views of 32x32 latents + the 64x128 panorama latent, SD-2-base widths, guidance 9, 90 degrees
    per step), 10 DDIM steps with the known band [112, 128) + [0, 40) of the panorama (and its e2p in the views) against
    tests/golden/cfg1_inpaint_ddim10.npz (the reference class as the denoiser, diffusers' blend in fp32 with the operands rolled
    with the state): views and panorama after EVERY step within 1e-3 rel-L2, the bar of the DDIM and 2M trajectories.  After
    result(), the kept entries are the known latents bit for bit.  Drift per step is printed with -s."""
    gd = golden("cfg1_inpaint_ddim10.npz")
    known = _fixture_known(gd)
    loop = _cfg1_loop(_hip_model(full_width), graphs, known)
    traj = _trajectory(loop)
    drift = [(rel_l2(v.cpu(), torch.from_numpy(gd["latents"][i])), rel_l2(p.cpu(), torch.from_numpy(gd["pano_latent"][i])))
             for i, (v, p) in enumerate(traj)]
    print("\ncfg1 10-step inpainting drift, graphs %s (views / pano rel-L2 per step):" % graphs)
    print("  " + "  ".join("%d: %.2e/%.2e" % (i + 1, a, b) for i, (a, b) in enumerate(drift)))
    lat, pano = loop.result()
    assert torch.equal(lat, traj[-1][0]) and torch.equal(pano, traj[-1][1])
    keep_v = (known.mask == 0).expand_as(lat)
    keep_p = (known.pano_mask == 0).expand_as(pano)
    assert int(keep_v.sum()) > 0 and int(keep_p.sum()) == 4 * 64 * 56
    assert torch.equal(lat[keep_v], known.latents[keep_v]) and torch.equal(pano[keep_p], known.pano_latent[keep_p])
    for i, (a, b) in enumerate(drift):
        assert a <= 1.0e-3 and b <= 1.0e-3, (i + 1, a, b)


def test_graph_replayed_known_2m_loop_equals_eager(full_width):
    """The blend runs in the two eager update launches outside the captured denoiser graphs, reading its operands by address: a
    graph-replayed 2M loop with known content and an eager one agree bit for bit after every step."""
    gd = golden("cfg1_inpaint_ddim10.npz")
    model = _hip_model(full_width)
    eager = _trajectory(_cfg1_loop(model, False, _fixture_known(gd), "dpmpp_2m"))
    graphed = _trajectory(_cfg1_loop(model, True, _fixture_known(gd), "dpmpp_2m"))
    for i, ((a, b), (c, d)) in enumerate(zip(eager, graphed)):
        assert torch.equal(a, c) and torch.equal(b, d), i + 1


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_mask_one_loop_is_the_plain_loop_bit_for_bit(full_width, sampler):
    """cfg 1 at full widths, 10 steps, graphs on: known content with m = 1 everywhere runs pf_cfg_inpaint_step_pair and must
    reproduce the known=None loop (pf_cfg_ddim_step_pair / pf_cfg_dpmpp_step_pair) exactly, after every step."""
    from panfusion_amd.pipeline import KnownRegion
    k = _fixture_known(golden("cfg1_inpaint_ddim10.npz"))
    ones = KnownRegion(k.latents, torch.ones_like(k.mask), k.pano_latent, torch.ones_like(k.pano_mask))
    model = _hip_model(full_width)
    plain = _trajectory(_cfg1_loop(model, True, None, sampler))
    one = _trajectory(_cfg1_loop(model, True, ones, sampler))
    for i, ((a, b), (c, d)) in enumerate(zip(plain, one)):
        assert torch.equal(a, c) and torch.equal(b, d), i + 1


# --------------------------------------------------------------------------------------------------------- builders
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


def _block_rule(gen):
    """Torch statement of the 8x8 rule: a latent pixel is generated (1) if any pixel of its block is (>= 0.5), kept (0) otherwise."""
    n, c, H, W = gen.shape
    return (gen >= 0.5).reshape(n, c, H // 8, 8, W // 8, 8).any(5).any(3).float()


def test_from_panorama_is_the_encoder_composition(tiny_encoder):
    from panfusion_amd.external.Perspective_and_Equirectangular import e2p
    from panfusion_amd.pipeline import KnownRegion
    from panfusion_amd.utils.pano import pad_pano, unpad_pano
    g = torch.Generator().manual_seed(12)
    pano = (torch.rand(1, 1, 3, 128, 256, generator=g) * 2 - 1).to(DEV)
    pmask = torch.ones(1, 1, 1, 128, 256)
    pmask[..., 200:] = 0.0
    pmask[..., :61] = 0.0                                 # not a multiple of 8: the partial block column is generated
    pmask[..., 30:40, 10:20] = 0.3                        # below 0.5: known (diffusers binarises at 0.5)
    pmask = pmask.to(DEV)
    cams = {k: v[None] for k, v in cam4().items()}
    k = KnownRegion.from_panorama(tiny_encoder, pano, pmask, cams, (8, 8))
    sf = tiny_encoder.packed(pano.device).scaling_factor
    want_p = unpad_pano(tiny_encoder.encode(pad_pano(pano[0], 64))[0], 8) * sf
    assert k.pano_latent.shape == (1, 1, 4, 16, 32) and torch.equal(k.pano_latent[0], want_p)
    flat = {n: v.reshape(-1) for n, v in cams.items()}
    crops = e2p(pano[0].expand(4, -1, -1, -1), flat["FoV"], flat["theta"], flat["phi"], (64, 64), mode="bilinear")
    assert k.latents.shape == (1, 4, 4, 8, 8) and torch.equal(k.latents[0], tiny_encoder.encode(crops)[0] * sf)
    want_pm = _block_rule(pmask[0])
    assert torch.equal(k.pano_mask[0], want_pm)
    assert want_pm[..., :7].eq(0).all() and want_pm[..., 7].eq(1).all() and want_pm[..., 25:].eq(0).all()
    mcrops = e2p(pmask[0].expand(4, -1, -1, -1), flat["FoV"], flat["theta"], flat["phi"], (64, 64), mode="nearest")
    assert k.mask.shape == (1, 4, 1, 8, 8) and torch.equal(k.mask[0], _block_rule(mcrops))
    assert 0 < float(k.mask.mean()) < 1


def test_from_view_keeps_exactly_the_covered_blocks(tiny_encoder):
    from panfusion_amd.external.Perspective_and_Equirectangular.p2e import p2e
    from panfusion_amd.pipeline import KnownRegion
    photo = (torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(13)) * 2 - 1).to(DEV)
    cams = {k: v[None] for k, v in cam4().items()}
    k = KnownRegion.from_view(tiny_encoder, photo, 90, 30.0, 10.0, cams, (16, 32), (8, 8))
    _, covered = p2e(photo, [90], [30.0], [10.0], (128, 256))
    kept = covered.reshape(1, 1, 16, 8, 32, 8).all(5).all(3)
    assert int(kept.sum()) > 0
    assert torch.equal(k.pano_mask[0] == 0, kept)
    assert set(k.pano_mask.unique().tolist()) <= {0.0, 1.0} and set(k.mask.unique().tolist()) <= {0.0, 1.0}


def test_cfg2_outpaint_from_a_photo(full_width, tiny_encoder):
    """cfg 2 geometry (20 icosahedron views of 64x64 latents + the 64x128 panorama latent, SD-2-base widths, graphs), 3 DDIM steps
    outpainting one synthetic 512x512 photo: everything finite, the kept region exact at the end."""
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion
    cams = FX.ico_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (64, 64), (64, 128))
    photo = (torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(14)) * 2 - 1).to(DEV)
    known = KnownRegion.from_view(tiny_encoder, photo, 90, 0.0, 0.0, cams, (64, 128), (64, 64))
    loop = DenoiseLoop(_hip_model(full_width), latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=3,
                       use_graphs=True, known=known)
    loop.prepare()
    lat, pano = loop.run()
    assert torch.isfinite(lat).all() and torch.isfinite(pano).all()
    keep_v = (known.mask == 0).expand_as(lat)
    keep_p = (known.pano_mask == 0).expand_as(pano)
    assert int(keep_v.sum()) > 0 and int(keep_p.sum()) > 0
    assert torch.equal(lat[keep_v], known.latents[keep_v].float()) and torch.equal(pano[keep_p], known.pano_latent[keep_p].float())
