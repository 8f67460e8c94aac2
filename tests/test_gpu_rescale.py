"""Guidance rescale on the MI355X: pf_cfg_moments and the factor of pf_cfg_rescaled_step_pair against float64,
the update against a float64 statement that uses the float64 factor, the bit-for-bit identities (phi = 0 against the existing
update kernels, no blend against mask = 1, a constant prediction), the refusals, the cfg 1 trajectory against the fixture
tools/make_golden_rescale.py wrote with the reference class as the denoiser and diffusers' rescale_noise_cfg in fp32, graph
replay against eager launches, and two short composed runs at the tiny widths.  Needs an MI355X: `-m gpu`."""
import pytest
import torch

from conftest import build_tiny_oracle, cam4, golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = 9.0


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def factor64(eu, ec, phi, samples, g=G):
    """f per sample in float64 from the fp32 predictions: phi std(eps_c) / std(eps_cfg) + 1 - phi, torch's own (unbiased) std."""
    c = ec.double().reshape(samples, -1)
    u = eu.double().reshape(samples, -1)
    return phi * c.std(1) / (u + g * (c - u)).std(1) + (1 - phi)


# ---------------------------------------------------------------------------------------- 1. moments and the factor
# (offset, scale) per sample, rotated over the shapes: a plain N(0, 1) prediction, a large one far from zero and a small one --
# an fp32 sum of squares loses the second, a sample index shared between two samples gives one of them another's statistics.
# |offset| <= 2 std(eps_c) in all of them: the per-element rounding of eps_cfg is relative to the VALUE, so its effect on
# sqrt(M2) is 6e-8 rms / std, and the 1e-6 below is the bound derived for rms / std of that order.
SPREADS = [(0.0, 1.0), (50.0, 30.0), (-0.02, 0.01)]
MOMENT_SHAPES = [(1, 2, 2), (1, 255, 255), (2, 4 * 7 * 9, 9), (3, 1000, 8), (2, 20 * 4 * 64 * 64, 64), (1, 4 * 64 * 128, 128)]


def _predictions(k, samples, elems):
    eu = rnd(samples, elems, seed=70 + k)
    ec = eu + 0.3 * rnd(samples, elems, seed=80 + k)
    off = torch.tensor([SPREADS[(k + s) % 3][0] for s in range(samples)])[:, None]
    sc = torch.tensor([SPREADS[(k + s) % 3][1] for s in range(samples)])[:, None]
    return (eu * sc + off).contiguous(), (ec * sc + off).contiguous()


@pytest.mark.parametrize("k", range(len(MOMENT_SHAPES)))
def test_moments_and_factor_vs_float64(k):
    """Every shape x n_partials in {1, 3, 64, 256} (more records than elements included): the records add up to the float64
    sums of eps_c (exact fp32 inputs: 1e-10 on the mean, relative to the rms, and on M2 -- float64 sums of <= 1280 terms per
    thread lose 1.4e-13, times (rms / std)^2 <= 4, on both sides; measured 0 and <= 1.1e-14) and of eps_cfg (sqrt(M2) to 1e-6);
    f from factor_out within 1e-6 relative of the float64 value (derived: 6e-8 from the fp32 rounding of eps_cfg,
    nothing from the float64 accumulation, 6e-8 from rounding f, times five; measured <= 6.4e-8); two launches into two buffers
    give the same bits; f moves by at most 1e-6 with n_partials (measured: not at all)."""
    from panfusion_amd import ops
    samples, elems, W = MOMENT_SHAPES[k]
    eu, ec = _predictions(k, samples, elems)
    phi = 0.7
    want = factor64(eu, ec, phi, samples)
    c64 = ec.double()
    mean64, m2_64 = c64.mean(1), ((c64 - c64.mean(1, keepdim=True)) ** 2).sum(1)
    e64 = eu.double() + G * (c64 - eu.double())
    m2_cfg64 = ((e64 - e64.mean(1, keepdim=True)) ** 2).sum(1)
    eud, ecd = eu.to(DEV), ec.to(DEV)
    x = rnd(samples, elems, seed=90 + k).to(DEV)
    fs = []
    for n_partials in (1, 3, 64, 256):
        a = ops.cfg_moments(eud, ecd, G, samples=samples, n_partials=n_partials)
        b = torch.full((samples, n_partials, 4), float("nan"), dtype=torch.float64, device=DEV)
        assert ops.cfg_moments(eud, ecd, G, samples=samples, out=b) is b
        assert a.shape == b.shape and a.dtype == torch.float64 and torch.equal(a, b)
        s = a.cpu().sum(1)
        mean, m2 = s[:, 0] / elems, s[:, 1] - s[:, 0] ** 2 / elems
        em, e2 = float(((mean - mean64) / (c64 ** 2).mean(1).sqrt()).abs().max()), float(((m2 - m2_64) / m2_64).abs().max())
        ecfg = float((((s[:, 3] - s[:, 2] ** 2 / elems) - m2_cfg64) / m2_cfg64).abs().max())
        assert ecfg <= 2e-6, (n_partials, ecfg)       # sqrt(M2_cfg) to 1e-6: the sample's own records, not a neighbour's
        f = torch.full((samples,), float("nan"), device=DEV)
        ops.cfg_rescaled_step_pair(x.view(-1, W), eud.view(-1, W), ecd.view(-1, W), G, (0.5, 0.8, 0.6, 0.7), partials=a, phi=phi,
                                   samples=samples, factor_out=f)
        ef = float(((f.cpu().double() - want) / want).abs().max())
        print("moments %s n_partials %d: mean %.1e  M2 %.1e  f %.2e (f = %s)" % (MOMENT_SHAPES[k], n_partials, em, e2, ef, f.tolist()))
        assert em <= 1e-10 and e2 <= 1e-10, (n_partials, em, e2)
        assert ef <= 1e-6, (n_partials, ef)
        fs.append(f.cpu().double())
    spread = float(((torch.stack(fs) - fs[0]) / fs[0]).abs().max())
    assert spread <= 1e-6, spread


# ---------------------------------------------------------------------------------------- 2. the update vs float64
def _masks(shape, seed):
    g = torch.Generator().manual_seed(seed)
    binary = (torch.rand(shape, generator=g) < 0.5).float()
    soft = torch.rand(shape, generator=g)
    soft[..., ::4] = binary[..., ::4]
    return soft


@pytest.mark.parametrize("shape", [(1, 20, 4, 64, 64), (1, 1, 4, 64, 128), (1, 1, 4, 128, 256)])
def test_rescaled_step_pair_vs_float64(shape):
    """The structure of test_inpaint_step_pair_vs_float64: cfg 2's view and panorama latents and a 256-wide panorama; (roll, phi,
    samples) = (0, 0.3, 1), (W/4, 0.7, 2), (17, 1.0, 1), (-5, 0.7, 2) -- two samples are the two halves of the rows, the second
    half three times as wide, offset and with a third of the guidance direction, so each half has its own f; the DDIM and 2M
    forms; with the blend (soft mask, known_roll 13) and without; in place and out of place.  out within 2e-6 rel-L2 -- the
    project's gate for these kernels -- of the float64 statement that uses the float64 f; out2 == out bit for bit; the timestep
    words written; x0_out within 2e-6 of the x0 of the rescaled eps."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DPMSolverSchedule
    sched = DPMSolverSchedule()
    sched.set_timesteps(50)
    W = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    x, hist = rnd(*shape, seed=41), rnd(*shape, seed=44) * 0.5
    half = torch.ones(rows, 1)
    half[rows // 2:] = 3.0
    eu = rnd(*shape, seed=42)
    ec = eu + (0.3 / half * rnd(rows, W, seed=43)).view(shape)         # a third of the guidance direction in the second half
    eu = (eu.view(rows, W) * half + (half - 1) * 0.4).view(shape).contiguous()
    ec = (ec.view(rows, W) * half + (half - 1) * 0.4).view(shape).contiguous()
    z, n, mask = rnd(*shape, seed=45), rnd(*shape, seed=46), _masks(shape, 47)
    d = lambda v: v.to(DEV)
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))
    kr = 13
    for form in ("ddim", "2m"):
        for i, roll, phi, samples in ((1, 0, 0.3, 1), (20, W // 4, 0.7, 2), (37, 17, 1.0, 1), (48, -5, 0.7, 2)):
            coef, k, order = sched.step_coefficients(i)
            ka, kb = coef[2:]
            sa, sb, sap, sbp = (torch.tensor(c, dtype=torch.float32).double() for c in coef)
            f64 = factor64(eu, ec, f32(phi), samples)
            if samples == 2:
                assert abs(float(f64[0] - f64[1])) > 1e-3
            eps = eu.double() + G * (ec.double() - eu.double())
            eps = (eps.view(samples, -1) * f64[:, None]).view(shape)
            x0 = (x.double() - sb * eps) / sa
            v = sap * x0 + sbp * eps
            if form == "2m":
                v = v + f32(k) * (x0 - hist.double())
            t_next = sched.timesteps[i + 1]
            part = ops.cfg_moments(d(eu), d(ec), G, samples=samples)
            for blend in (False, True):
                r = lambda t: torch.roll(t.double(), kr, -1)
                vb = r(mask) * v + (1 - r(mask)) * (f32(ka) * r(z) + f32(kb) * r(n)) if blend else v
                want, want_x0 = torch.roll(vb, roll, -1), torch.roll(x0, roll, -1)
                bl = dict(known=d(z), noise=d(n), mask=d(mask), ka=ka, kb=kb, known_roll=kr) if blend else {}
                for in_place in (False, True):
                    pair = torch.stack([x[0], x[0]]).to(DEV)
                    h = d(hist)
                    tstep = torch.full((2, 5), 7, dtype=torch.long, device=DEV)
                    fo = torch.zeros(samples, device=DEV)
                    hx = dict(x0_prev=h, k=k, x0_out=h) if form == "2m" else {}
                    common = dict(tstep=tstep, t_next=t_next, partials=part, phi=phi, samples=samples, factor_out=fo)
                    if in_place:
                        out, x0_out = ops.cfg_rescaled_step_pair(pair[:1], d(eu), d(ec), G, coef, roll, out=pair[:1],
                                                                 out2=pair[1:], **common, **hx, **bl)
                        assert out.data_ptr() == pair.data_ptr()
                        out2 = pair[1:]
                    else:
                        out2 = torch.empty_like(pair[1:])
                        if form == "2m":
                            hx["x0_out"] = torch.empty_like(h)
                        out, x0_out = ops.cfg_rescaled_step_pair(d(x), d(eu), d(ec), G, coef, roll, out2=out2, **common, **hx, **bl)
                    e = rel_l2(out.cpu(), want)
                    assert e <= 2e-6, (shape, form, i, roll, phi, samples, blend, in_place, e)
                    assert torch.equal(out2, out)
                    assert torch.equal(tstep.cpu(), torch.full((2, 5), t_next, dtype=torch.long))
                    assert float(((fo.cpu().double() - f64) / f64).abs().max()) <= 1e-6
                    if form == "2m":
                        e0 = rel_l2(x0_out.cpu(), want_x0)
                        assert e0 <= 2e-6, (shape, i, roll, phi, samples, blend, in_place, e0)
                    else:
                        assert x0_out is None


# ---------------------------------------------------------------------------------------- 3. identities, bit for bit
@pytest.mark.parametrize("shape", [(1, 20, 4, 64, 64), (1, 1, 4, 64, 128), (1, 3, 4, 7, 9)])
def test_identities_bit_for_bit(shape):
    """phi = 0 through the new entry point, moments launched: f is exactly 1 and the outputs are those of pf_cfg_ddim_step_pair,
    pf_cfg_dpmpp_step_pair and pf_cfg_inpaint_step_pair (both forms).  No blend (NULL operands) == the blend with mask = 1, at
    phi = 0.7.  A constant prediction (0.25 everywhere): f = 1, finite output equal to the plain update."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DPMSolverSchedule
    sched = DPMSolverSchedule()
    sched.set_timesteps(20)
    W = shape[-1]
    x, eu, ec, hist, z, n = (rnd(*shape, seed=51 + j).to(DEV) for j in range(6))
    mask = _masks(shape, 57).to(DEV)
    ones = torch.ones_like(x)
    part = ops.cfg_moments(eu, ec, G, samples=1)
    for i, roll, kr in ((3, 0, 0), (7, W // 4, W // 4), (11, -5, 13), (18, 17, W - 1)):
        coef, k, _ = sched.step_coefficients(i)
        fo = torch.zeros(1, device=DEV)
        rs = dict(partials=part, phi=0.0, factor_out=fo)
        bl = dict(known=z, noise=n, ka=coef[2], kb=coef[3], known_roll=kr)
        h2 = lambda: dict(x0_prev=hist, k=k, x0_out=torch.empty_like(x))
        got, none = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, **rs)
        assert none is None and torch.equal(got, ops.cfg_ddim_step_pair(x, eu, ec, G, coef, roll))
        assert float(fo) == 1.0
        got, got_x0 = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, **h2(), **rs)
        want, want_x0 = ops.cfg_dpmpp_step_pair(x, eu, ec, G, coef, roll, x0_prev=hist, k=k)
        assert torch.equal(got, want) and torch.equal(got_x0, want_x0)
        got, _ = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, mask=mask, **bl, **rs)
        assert torch.equal(got, ops.cfg_inpaint_step_pair(x, eu, ec, G, coef, roll, mask=mask, **bl)[0])
        got, got_x0 = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, mask=mask, **h2(), **bl, **rs)
        want, want_x0 = ops.cfg_inpaint_step_pair(x, eu, ec, G, coef, roll, mask=mask, **h2(), **bl)
        assert torch.equal(got, want) and torch.equal(got_x0, want_x0)
        # no blend == mask 1
        rs = dict(partials=part, phi=0.7, factor_out=fo)
        a, _ = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, **rs)
        b, _ = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, mask=ones, **bl, **rs)
        assert torch.equal(a, b) and float(fo) != 1.0
        a, a0 = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, **h2(), **rs)
        b, b0 = ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, roll, mask=ones, **h2(), **bl, **rs)
        assert torch.equal(a, b) and torch.equal(a0, b0)
    const = torch.full_like(x, 0.25)
    fo = torch.zeros(1, device=DEV)
    cp = ops.cfg_moments(const, const, G, samples=1)
    got, _ = ops.cfg_rescaled_step_pair(x, const, const, G, coef, 5, partials=cp, phi=0.7, factor_out=fo)
    assert float(fo) == 1.0 and torch.isfinite(got).all()
    assert torch.equal(got, ops.cfg_ddim_step_pair(x, const, const, G, coef, 5))


# ---------------------------------------------------------------------------------------------- 4. bad arguments
def test_rescale_ops_reject_bad_arguments():
    from panfusion_amd import _lib, ops
    coef = (0.5, 0.8, 0.6, 0.7)
    x, eu, ec, h, z, n, m = (torch.zeros(1, 4, 8, 64, device=DEV) for _ in range(7))
    out = torch.empty_like(x)
    part = torch.zeros(1, 64, 4, dtype=torch.float64, device=DEV)
    ok = dict(partials=part, phi=0.7)
    blend = dict(known=z, noise=n, mask=m, ka=0.6, kb=0.7, known_roll=5)
    E = _lib.PanFusionHipError
    with pytest.raises(E, match="sample_rows"):
        ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, samples=3, partials=torch.zeros(3, 64, 4, dtype=torch.float64, device=DEV), phi=0.7)
    for phi in (-0.1, 1.5, float("nan")):
        with pytest.raises(E, match="phi"):
            ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, partials=part, phi=phi)
    with pytest.raises(E, match="partials"):
        ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, partials=None, phi=0.7)
    with pytest.raises(E, match="n_partials"):
        ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, partials=torch.zeros(1, 257, 4, dtype=torch.float64, device=DEV), phi=0.7)
    with pytest.raises(E, match="n_partials"):
        ops.cfg_moments(eu, ec, G, samples=1, n_partials=257)
    with pytest.raises(E, match="sample_elems"):
        ops.cfg_moments(eu.view(-1)[:3], ec.view(-1)[:3], G, samples=3, n_partials=4)
    # known / noise / mask together or not at all, and what the inpaint entry point refuses
    for name in ("known", "noise", "mask"):
        with pytest.raises(E, match="together"):
            ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, 3, out=out, **dict(blend, **{name: None}), **ok)
    wide = torch.zeros(1, 8193, device=DEV)
    with pytest.raises(E, match="8192"):
        ops.cfg_rescaled_step_pair(wide, wide.clone(), wide.clone(), G, coef, x0_out=wide.clone(), **ok)
    wider = torch.zeros(1, 16385, device=DEV)
    with pytest.raises(E, match="16384"):
        ops.cfg_rescaled_step_pair(wider, wider.clone(), wider.clone(), G, coef, **ok)
    bad = [dict(out=out, **dict(blend, noise=out)), dict(out=out, **dict(blend, known=out)),
           dict(out=out, x0_out=h, **dict(blend, mask=h)), dict(out=out, x0_prev=h, **blend), dict(out=out, x0_prev=h),
           dict(out=out, x0_out=out, **blend), dict(out=x, out2=x, **blend), dict(out=x, out2=x), dict(out=eu)]
    for kw in bad:
        with pytest.raises(E):
            ops.cfg_rescaled_step_pair(x, eu, ec, G, coef, 3, **kw, **ok)
    torch.cuda.synchronize()                          # nothing was launched, nothing is pending
    assert _lib.lib().pf_last_error_string()


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


def _cfg1_loop(model, graphs, phi, prompt_scale, sampler="ddim", steps=10):
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    pe, ppe = torch.cat([pe[:1], pe[1:] * prompt_scale]), torch.cat([ppe[:1], ppe[1:] * prompt_scale])
    kw = {} if phi is None else dict(guidance_rescale=phi)
    return DenoiseLoop(model, latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=steps,
                       use_graphs=graphs, sampler=sampler, **kw)


def _trajectory(loop, n=None):
    """(views, panorama in the un-rotated frame, factors) after every step."""
    from panfusion_amd import ops
    traj = []
    for _ in range(n or len(loop.timesteps)):
        loop.step()
        f = None if loop.rescale_factors is None else loop.rescale_factors.clone()
        traj.append((loop.lat.clone(), ops.roll_width(loop.pano, int(-loop.total_rot / 360 * loop.W)).clone(), f))
    return traj


@pytest.mark.parametrize("graphs", [True, False])
def test_cfg1_ten_rescaled_steps_vs_oracle(full_width, graphs):
    """BASELINE.json configs[0] (m = 4 views of 32x32 latents + the 64x128 panorama latent, SD-2-base widths, guidance 9, 90
    degrees per step), 10 DDIM steps with guidance_rescale = 0.7 against tests/golden/cfg1_rescale_ddim10.npz (the reference
    class as the denoiser, diffusers' rescale_noise_cfg in fp32 before scheduler.step; the conditional prompt scaled by the
    constant in the fixture): views and panorama after EVERY step within 1e-3 rel-L2, the gate of every cfg 1 trajectory here.
    The same loop with guidance_rescale = 0 misses the fixture by more than 1e-2 at the last step.  The factor error is
    printed, not gated (a ratio of two norms that each carry the model's parity error).  Drift per step is printed with -s."""
    gd = golden("cfg1_rescale_ddim10.npz")
    scale, phi = float(gd["prompt_scale"]), float(gd["phi"])
    assert abs(phi - 0.7) < 1e-6
    fx = torch.from_numpy(gd["factors"]).double()
    assert fx.shape == (10, 2) and bool((((fx < 0.98) | (fx > 1.02)).any(1)).all())       # the fixture does discriminate
    model = _hip_model(full_width)
    traj = _trajectory(_cfg1_loop(model, graphs, 0.7, scale))
    drift = [(rel_l2(v.cpu(), torch.from_numpy(gd["latents"][i])), rel_l2(p.cpu(), torch.from_numpy(gd["pano_latent"][i])))
             for i, (v, p, _) in enumerate(traj)]
    ferr = [float(((f.cpu().double() - fx[i]) / fx[i]).abs().max()) for i, (_, _, f) in enumerate(traj)]
    print("\ncfg1 10-step rescaled drift, graphs %s (views / pano rel-L2 per step):" % graphs)
    print("  " + "  ".join("%d: %.2e/%.2e" % (i + 1, a, b) for i, (a, b) in enumerate(drift)))
    print("  factor error per step (relative, max of the two): " + "  ".join("%.2e" % e for e in ferr))
    print("  largest: drift %.2e  factor %.2e" % (max(max(d) for d in drift), max(ferr)))
    for i, (a, b) in enumerate(drift):
        assert a <= 1.0e-3 and b <= 1.0e-3, (i + 1, a, b)
    plain = _trajectory(_cfg1_loop(model, graphs, 0.0, scale))
    miss = (rel_l2(plain[-1][0].cpu(), torch.from_numpy(gd["latents"][-1])),
            rel_l2(plain[-1][1].cpu(), torch.from_numpy(gd["pano_latent"][-1])))
    print("  guidance_rescale = 0 against the fixture at the last step: %.2e/%.2e" % miss)
    assert min(miss) > 1e-2, miss


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_graph_replayed_rescaled_loop_equals_eager(full_width, sampler):
    """The two extra launches per latent run eagerly between graph replays and read the graph's outputs by address: 5 steps,
    state and factors bit for bit."""
    scale = float(golden("cfg1_rescale_ddim10.npz")["prompt_scale"])
    model = _hip_model(full_width)
    eager = _trajectory(_cfg1_loop(model, False, 0.7, scale, sampler), 5)
    graphed = _trajectory(_cfg1_loop(model, True, 0.7, scale, sampler), 5)
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert all(torch.equal(s, t) for s, t in zip(a, b)), i + 1


@pytest.fixture(scope="module")
def tiny_model():
    from panfusion_amd.models.pano import MultiViewBaseModel
    om = build_tiny_oracle()
    m = MultiViewBaseModel(om.unet, om.pano_unet, None, None, om.pano_pad, compute_dtype=torch.float16)
    m.load_state_dict({k: v for k, v in om.state_dict().items() if k.startswith("cp_blocks")}, strict=False)
    return m


def _tiny_inputs():
    g = golden("mvgen_tiny.npz")
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    return t("latents")[:1], t("pano_latent")[:1], t("prompt_embd"), t("pano_prompt_embd"), {k: v[None] for k, v in cam4().items()}


def test_composed_2m_known_strength_rescale_run(tiny_model):
    """2M + known region + strength 0.5 + rescale at the tiny widths: finite, factors written, a second identical run (a fresh
    loop, and the same loop restarted) equals the first bit for bit."""
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion
    lat, pano, pe, ppe, cams = _tiny_inputs()
    W = pano.shape[-1]
    mask_p = torch.ones(1, 1, 1, *pano.shape[-2:], device=DEV)
    mask_p[..., W - 4:] = 0.0
    mask_p[..., :10] = 0.0
    mask_v = torch.ones(1, lat.shape[1], 1, *lat.shape[-2:], device=DEV)
    mask_v[..., :5] = 0.0
    known = KnownRegion(rnd(*lat.shape, seed=61).to(DEV), mask_v, rnd(*pano.shape, seed=62).to(DEV), mask_p)
    make = lambda: DenoiseLoop(tiny_model, lat, pano, pe, ppe, cams, steps=6, sampler="dpmpp_2m", known=known, strength=0.5,
                               guidance_rescale=0.7)
    loop = make()
    first = [t.clone() for t in loop.run()]
    f = loop.rescale_factors.clone()
    assert loop.i == 3 and all(torch.isfinite(t).all() for t in first) and torch.isfinite(f).all() and bool((f != 1).all())
    keep = (mask_p == 0).expand_as(first[1])
    assert torch.equal(first[1][keep], known.pano_latent[keep])
    again = make()
    assert all(torch.equal(a, b) for a, b in zip(again.run(), first)) and torch.equal(again.rescale_factors, f)
    loop.restart()
    assert all(torch.equal(a, b) for a, b in zip(loop.run(), first)) and torch.equal(loop.rescale_factors, f)


def test_hires_loop_with_rescale(tiny_model):
    """HiResLoop forwards guidance_rescale to both of its loops: tiny widths, 16x32 -> 32x64 panorama, 3 + 2 steps, finite, and
    a second identical run equals the first bit for bit; without the argument the result differs."""
    from oracle import ddim as oddim
    from panfusion_amd.pipeline import HiResLoop
    lat, pano, pe, ppe, cams = _tiny_inputs()
    n_pano = rnd(1, 1, 4, 2 * pano.shape[-2], 2 * pano.shape[-1], seed=63)
    n_lat = oddim.init_noise(n_pano, cams, *lat.shape[-2:])[1]
    make = lambda **kw: HiResLoop(tiny_model, (lat, pano), (n_lat.to(DEV), n_pano.to(DEV)), pe, ppe, cams, steps=3, refine_steps=4,
                                  strength=0.5, **kw)
    a = make(guidance_rescale=0.7)
    assert a.base.rescale == a.refine.rescale == 0.7
    first = [t.clone() for t in a.run()]
    assert all(torch.isfinite(t).all() for t in first) and first[1].shape == n_pano.shape
    assert torch.isfinite(a.base.rescale_factors).all() and torch.isfinite(a.refine.rescale_factors).all()
    assert all(torch.equal(x, y) for x, y in zip(make(guidance_rescale=0.7).run(), first))
    assert not any(torch.equal(x, y) for x, y in zip(make().run(), first))
