"""Guidance rescale, host side: the torch stand-ins of the two new ops against a literal transcription of
diffusers' rescale_noise_cfg in float64, the loop on the test double tests/fake_ops.py against a hand-written loop that applies
the transcription before oracle.ddim's update (DDIM and 2M, with and without known content, strength 1 and 0.5),
guidance_rescale=0 against the loop built without the argument (no call of either new op), restart() against a fresh loop, the
sharded loop over gloo, the ValueErrors, and the C entry points' argument checks (no launch, no GPU)."""
import ctypes as C
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fake_ops
from conftest import build_tiny_oracle, rel_l2
from test_inpaint_cpu import _inputs, _known
from test_strength_cpu import START_OP, _source, get_timesteps
from test_strength_cpu import _use_fake_backend as _strength_backend

HERE = os.path.dirname(os.path.abspath(__file__))
CALLS = {"moments": 0, "step": 0}
PARTIALS, DOUBLES = 64, 4


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers 0.24 pipeline_stable_diffusion.py: rescale_noise_cfg, literally."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    # rescale the results from guidance (fixes overexposure)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    # mix with the original results from guidance by factor guidance_rescale to avoid "plain looking" images
    noise_cfg = guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg
    return noise_cfg


# ------------------------------------------------------------------------------------------------- the stand-ins
def cfg_moments(eps_uncond, eps_cond, guidance, *, samples, out=None, n_partials=None):
    """Torch stand-in for ops.cfg_moments, set on the fake_ops module at run time: the four float64 sums of every sample in its
    record 0, zeros in the others (the consumer adds all records)."""
    CALLS["moments"] += 1
    c = eps_cond.double().reshape(samples, -1)
    e = (eps_uncond + guidance * (eps_cond - eps_uncond)).double().reshape(samples, -1)
    if out is None:
        out = torch.empty(samples, n_partials or PARTIALS, DOUBLES, dtype=torch.float64)
    out.zero_()
    out.view(samples, -1, DOUBLES)[:, 0] = torch.stack([c.sum(1), (c * c).sum(1), e.sum(1), (e * e).sum(1)], 1)
    return out


def rescale_factor(partials, samples, n, phi):
    """f per sample from the records, in float64: phi sqrt(M2_text / M2_cfg) + 1 - phi, 1 where M2_cfg <= 0."""
    s = partials.view(samples, -1, DOUBLES).sum(1)
    m2_text = (s[:, 1] - s[:, 0] ** 2 / n).clamp_min(0)
    m2_cfg = s[:, 3] - s[:, 2] ** 2 / n
    f = phi * (m2_text / m2_cfg).sqrt() + (1 - phi)
    return torch.where(m2_cfg > 0, f, torch.ones_like(f))


def cfg_rescaled_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                           x0_prev=None, k=0.0, x0_out=None, *, partials, phi, samples=1, factor_out=None,
                           known=None, noise=None, mask=None, ka=0.0, kb=0.0, known_roll=0):
    """Torch stand-in for ops.cfg_rescaled_step_pair: eps = f (u + g (c - u)) with f from the records, then the arithmetic of
    the stand-ins of the other update ops (test_inpaint_cpu.cfg_inpaint_step_pair), the blend only with known content."""
    CALLS["step"] += 1
    sa, sb, sap, sbp = coef
    f = rescale_factor(partials, samples, x.numel() // samples, phi)
    eps = eps_uncond + guidance * (eps_cond - eps_uncond)
    eps = (eps.reshape(samples, -1) * f.to(eps.dtype)[:, None]).reshape(eps.shape)
    x0 = (x - sb * eps) / sa
    y = sap * x0 + sbp * eps
    if x0_prev is not None:
        y = y + k * (x0 - x0_prev)
    if known is not None:
        z, n, m = (torch.roll(t, known_roll, -1) for t in (known, noise, mask))
        y = m * y + (1 - m) * (ka * z + kb * n)
    y = torch.roll(y, roll, -1)
    out = y if out is None else out.copy_(y)
    if out2 is not None:
        out2.copy_(y)
    if x0_out is not None:
        x0_out.copy_(torch.roll(x0, roll, -1))
    if tstep is not None:
        tstep.fill_(int(t_next))
    if factor_out is not None:
        factor_out[:samples].copy_(f)
    return out, x0_out


def _use_fake_backend(put, extra=()):
    _strength_backend(put, extra)
    put(fake_ops, "cfg_moments", cfg_moments)
    put(fake_ops, "cfg_rescaled_step_pair", cfg_rescaled_step_pair)
    put(fake_ops, "CFG_PARTIALS", PARTIALS)
    put(fake_ops, "CFG_MOMENT_DOUBLES", DOUBLES)


@pytest.fixture
def fake_backend(monkeypatch):
    _use_fake_backend(lambda o, n, v: monkeypatch.setattr(o, n, v, raising=False), ["panfusion_amd.sharding"])
    monkeypatch.setitem(START_OP, "enabled", True)
    monkeypatch.setitem(START_OP, "calls", [])
    monkeypatch.setitem(CALLS, "moments", 0)
    monkeypatch.setitem(CALLS, "step", 0)
    return monkeypatch


@pytest.fixture(scope="module")
def oracle_model():
    return build_tiny_oracle()


# ------------------------------------------------------------------------------- the stand-in is rescale_noise_cfg
@pytest.mark.parametrize("phi", [0.0, 0.3, 0.7, 1.0])
def test_stand_in_is_rescale_noise_cfg(phi):
    """float64 on both sides, random (2, 3, 4, 8, 8) predictions with a different spread and offset per sample: 1e-12."""
    g = torch.Generator().manual_seed(31)
    shape = (2, 3, 4, 8, 8)
    eu = torch.randn(shape, generator=g, dtype=torch.float64)
    ec = eu + 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    scale = torch.tensor([1.0, 4.0], dtype=torch.float64).reshape(2, 1, 1, 1, 1)
    eu, ec = eu * scale + 0.2, ec * scale + 0.2
    want = rescale_noise_cfg(eu + 9.0 * (ec - eu), ec, phi)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    part = cfg_moments(eu, ec, 9.0, samples=2)
    assert part.shape == (2, PARTIALS, DOUBLES) and part.dtype == torch.float64
    f = rescale_factor(part, 2, eu[0].numel(), phi)
    got = (eu + 9.0 * (ec - eu)) * f.reshape(2, 1, 1, 1, 1)
    assert rel_l2(got, want) < 1e-12 and float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    # and through the update op: (sa, sb, sap, sbp) = (1, 0, 0, 1) returns eps itself
    fo = torch.zeros(2, dtype=torch.float64)
    out, _ = cfg_rescaled_step_pair(x, eu, ec, 9.0, (1.0, 0.0, 0.0, 1.0), partials=part, phi=phi, samples=2, factor_out=fo)
    assert rel_l2(out, want) < 1e-12 and torch.equal(fo, f)
    if phi == 0.0:
        assert torch.equal(f, torch.ones(2, dtype=torch.float64))
    # a constant prediction: NaN in diffusers, f = 1 here
    c = torch.full(shape, 0.25, dtype=torch.float64)
    assert torch.isnan(rescale_noise_cfg(c, c, 0.7)).all()
    assert torch.equal(rescale_factor(cfg_moments(c, c, 9.0, samples=2), 2, c[0].numel(), 0.7), torch.ones(2, dtype=torch.float64))


# ------------------------------------------------------------------------------------------ the loop on the fake backend
def restated(model, n_v, n_p, pe, ppe, cams, z_v, z_p, known, steps, strength, sampler, phi, rot_diff=90.0, guidance=9.0):
    """PanFusion.inference's loop (PanFusion.py:146-164) with rescale_noise_cfg applied to the merged predictions before the
    scheduler's update -- oracle.ddim's DDIM.step, or 2M in diffusers' form -- and, with known content, diffusers' blend; the
    start below strength 1 is add_noise at the first sliced timestep.  Everything of the panorama is rolled with torch.roll.
    Returns the (views, panorama in the state's own frame) after every step."""
    from oracle import ddim as oddim
    ddim = oddim.DDIM()
    ac = ddim.alphas_cumprod
    full = [int(t) for t in ddim.set_timesteps(steps)]
    ts, k = get_timesteps(full, steps, strength)
    i0 = steps - k
    a_s = lambda t: ((ac[t] if t >= 0 else ac[0]) ** 0.5, (1 - (ac[t] if t >= 0 else ac[0])) ** 0.5)
    lam = lambda t: torch.log(a_s(t)[0]) - torch.log(a_s(t)[1])
    add_noise = lambda z, n, t: ac[t] ** 0.5 * z + (1 - ac[t]) ** 0.5 * n
    shift = int(rot_diff / 360 * n_p.shape[-1])
    roll = lambda t: torch.roll(t, shift, -1)
    latents, pano = (add_noise(z_v, n_v, ts[0]), add_noise(z_p, n_p, ts[0])) if strength < 1 else (n_v.clone(), n_p.clone())
    if known is not None:
        m_v, m_p = known.mask, known.pano_mask
    x0_v = x0_p = None
    traj = []
    m = latents.shape[1]
    for j, s0 in enumerate(ts):
        i = i0 + j
        pano, cams = oddim.rotate_latent(pano, cams, rot_diff)
        z_p, n_p = roll(z_p), roll(n_p)
        m_p = roll(m_p) if known is not None else None
        x0_p = None if x0_p is None else roll(x0_p)
        with torch.no_grad():
            e, pe_ = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano), torch.full((2, m), s0, dtype=torch.long), pe, ppe,
                           oddim.cfg_pair(cams))
        t = s0 - 1000 // steps
        (al_s, sg_s), (al_t, sg_t) = a_s(s0), a_s(t)
        h = lam(t) - lam(s0)
        second = sampler == "dpmpp_2m" and j > 0 and not (i == steps - 1 and steps < 15)
        last = j == len(ts) - 1
        new = []
        for x, pred, x0_prev, z, mk, n in ((latents, e, x0_v, z_v, m_v if known is not None else None, n_v),
                                           (pano, pe_, x0_p, z_p, m_p, n_p)):
            eps = rescale_noise_cfg(oddim.cfg_merge(pred, guidance), pred.chunk(2)[1], phi)     # (b, m, 4, h, w): dims 1..
            if sampler == "ddim":
                y, x0 = ddim.step(eps, s0, x), None
            else:
                x0 = (x - sg_s * eps) / al_s
                y = (sg_t / sg_s) * x - (al_t * (torch.exp(-h) - 1.0)) * x0
                if second:
                    r0 = (lam(s0) - lam(full[i - 1])) / h
                    y = y - 0.5 * (al_t * (torch.exp(-h) - 1.0)) * ((1.0 / r0) * (x0 - x0_prev))
            if known is not None:
                proper = z if last else add_noise(z, n, ts[j + 1])
                y = (1 - mk) * proper + mk * y
            new.append((y, x0))
        (latents, x0_v), (pano, x0_p) = new
        traj.append((latents, pano))
    return traj


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("with_known", [False, True])
@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_rescaled_loop_matches_hand_written_loop(fake_backend, oracle_model, sampler, with_known, strength):
    """6 steps (3 at strength 0.5), phi = 0.7: the state after every step equals the hand-written loop within 1e-4 rel-L2, the
    bound of the same comparison in test_inpaint_cpu / test_strength_cpu (fp32 on both sides); per step one call of each new
    op per latent, none of the other update ops; the factors are the transcription's std ratio."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    steps, phi = 6, 0.7
    lat, pano, pe, ppe, cams = _inputs()
    known = _known(lat, pano, cams) if with_known else None
    src = _source(lat, pano, cams)
    z = (known.latents, known.pano_latent) if with_known else (src.latents, src.pano_latent)
    want = restated(oracle_model, lat, pano, pe, ppe, cams, z[0], z[1], known, steps, strength, sampler, phi)
    for name in ("cfg_ddim_step_pair", "cfg_dpmpp_step_pair", "cfg_inpaint_step_pair"):
        def never(*a, _n=name, **kw):
            raise AssertionError("%s called by a rescaled loop" % _n)
        fake_backend.setattr(fake_ops, name, never)
    loop = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=steps, sampler=sampler, known=known,
                       strength=strength, init=None if (with_known or strength == 1.0) else src, guidance_rescale=phi)
    assert len(loop.timesteps) == len(want) == int(steps * strength)
    assert loop.rescale_factors.shape == (2,) and loop.rescale_factors.dtype == torch.float32
    seen = []
    for j in range(len(want)):
        loop.step()
        moved = 0 if j == len(want) - 1 else loop.shift
        ev, ep = rel_l2(loop.lat, want[j][0]), rel_l2(torch.roll(loop.pano, -moved, -1), want[j][1])
        assert ev < 1e-4 and ep < 1e-4, (sampler, with_known, strength, j + 1, ev, ep)
        seen.append(loop.rescale_factors.clone())
    assert CALLS["moments"] == CALLS["step"] == 2 * len(want)
    assert all(torch.isfinite(f).all() and float((f - 1).abs().max()) > 1e-3 for f in seen)      # the feature is in effect


def test_rescale_really_changes_the_run(fake_backend, oracle_model):
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    a = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3)
    b = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, guidance_rescale=0.7)
    a.step()
    b.step()
    assert rel_l2(b.lat, a.lat) > 1e-2 and rel_l2(b.pano, a.pano) > 1e-2


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("with_known", [False, True])
def test_rescale_zero_is_the_loop_without_the_argument(fake_backend, oracle_model, sampler, with_known):
    """guidance_rescale=0 (given or defaulted): no call of either new op, no buffers, and a run bit-identical to the loop built
    without the argument."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    known = _known(lat, pano, cams) if with_known else None
    make = lambda **kw: DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, sampler=sampler, known=known, **kw)
    a, b, c = make(), make(guidance_rescale=0.0), make(guidance_rescale=0)
    assert b.rescale_factors is None and not hasattr(b, "_moments_lat")
    for _ in range(3):
        for loop in (a, b, c):
            loop.step()
        for loop in (b, c):
            assert torch.equal(a.lat2, loop.lat2) and torch.equal(a.pano2, loop.pano2) and torch.equal(a.tstep, loop.tstep)
    assert all(torch.equal(x, y) for x, y in zip(a.result(), b.result()))
    assert CALLS == {"moments": 0, "step": 0}


# ------------------------------------------------------------------------------------------------------- restart()
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_restarted_rescaled_loop_equals_a_fresh_one(fake_backend, oracle_model, sampler):
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    known, src = _known(lat, pano, cams), _source(lat, pano, cams)
    model = hip_model(oracle_model)
    make = lambda **kw: DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=5, sampler=sampler, guidance_rescale=0.7,
                                    **dict(dict(known=known, strength=0.8, init=src), **kw))
    loop = make()
    bufs = [t.data_ptr() for t in (loop._moments_lat, loop._moments_pano, loop.rescale_factors)]
    want = [t.clone() for t in make().run()]
    for _ in range(2):
        loop.step()
    loop.restart()
    assert loop.rescale == 0.7
    assert _same(loop.run(), want)
    loop.restart(strength=0.4)
    assert _same(loop.run(), make(strength=0.4).run())
    assert bufs == [t.data_ptr() for t in (loop._moments_lat, loop._moments_pano, loop.rescale_factors)]
    assert not _same(want, DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=5, sampler=sampler, known=known, strength=0.8,
                                       init=src).run())


def test_hires_loop_forwards_the_argument(fake_backend):
    from panfusion_amd.pipeline import HiResLoop
    lat, pano, pe, ppe, cams = _inputs()
    model = lambda lat2, pano2, *a: (torch.zeros_like(lat2), torch.zeros_like(pano2))
    hr = HiResLoop(model, (lat, pano), (lat, pano), pe, ppe, cams, steps=4, strength=0.5, guidance_rescale=0.3)
    assert hr.base.rescale == hr.refine.rescale == 0.3
    assert hr.base.rescale_factors is not hr.refine.rescale_factors
    hr = HiResLoop(model, (lat, pano), (lat, pano), pe, ppe, cams, steps=4, strength=0.5)
    assert hr.base.rescale == hr.refine.rescale == 0.0
    with pytest.raises(ValueError):
        HiResLoop(model, (lat, pano), (lat, pano), pe, ppe, cams, steps=4, strength=0.5, guidance_rescale=1.5)


# --------------------------------------------------------------------------------------- sharded loop over gloo
def _scenario(make):
    lat, pano, pe, ppe, cams = args = _inputs()
    loop = make(args, steps=3, sampler="dpmpp_2m", known=_known(lat, pano, cams), guidance_rescale=0.7)
    out = [t.clone() for t in loop.run()]
    return out + [loop.rescale_factors.clone()]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    _use_fake_backend(setattr, ["panfusion_amd.sharding"])
    START_OP["enabled"] = True
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from panfusion_amd import sharding
        from test_engine_logic_cpu import hip_model
        model = hip_model(build_tiny_oracle())
        make = lambda args, **kw: sharding.ShardedDenoiseLoop(model, sharding.make_shard(4), *args, **kw)
        torch.save(_scenario(make), os.path.join(out, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_rescaled_loop_equals_single_process(fake_backend):
    """World 2: every rank holds the full gathered predictions of both latents, so each computes the same statistics: the
    replicas are bit-identical and equal the single-process loop (1e-4, the bound of the other sharded loop tests)."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    from test_sharding_gloo import _free_port
    world = 2
    model = hip_model(build_tiny_oracle())
    want = _scenario(lambda args, **kw: DenoiseLoop(model, *args, **kw))
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    for r in res:
        assert rel_l2(r[0], want[0]) < 1e-4 and rel_l2(r[1], want[1]) < 1e-4 and rel_l2(r[2], want[2]) < 1e-4
    assert _same(res[0], res[1])


# ---------------------------------------------------------------------------------------------------- bad inputs
def test_loop_rejects_bad_guidance_rescale(fake_backend):
    from panfusion_amd.pipeline import DenoiseLoop
    lat, pano, pe, ppe, cams = _inputs()
    for phi in (-0.1, 1.0001, 2, float("nan"), float("inf"), -float("inf"), None, "0.5"):
        with pytest.raises(ValueError, match="guidance_rescale"):
            DenoiseLoop(None, lat, pano, pe, ppe, cams, steps=4, guidance_rescale=phi)
    for phi in (0, 0.0, 0.5, 1, 1.0):
        assert DenoiseLoop(None, lat, pano, pe, ppe, cams, steps=4, guidance_rescale=phi).rescale == float(phi)


# ------------------------------------------------------------------------------------- C entry points: argument checks
def test_entry_points_reject_bad_arguments_before_launching():
    """Validation happens before any launch (fake, never dereferenced device addresses; every call below must fail), and the
    message names the argument."""
    from panfusion_amd import _lib
    lib = _lib.lib()
    X, EU, EC, OUT, OUT2, H0, H1, Z, N, M, P, F = (0x10000 * i for i in range(1, 13))
    err = lib.pf_last_error_string

    def moments(eu=EU, ec=EC, n_samples=2, elems=100, part=P, n_partials=64):
        return lib.pf_cfg_moments(eu, ec, C.c_float(9.0), n_samples, elems, part, n_partials, None)
    assert moments(part=None) == 1 and b"partials" in err()
    assert moments(eu=None) == 1 and moments(ec=None) == 1
    assert moments(n_partials=0) == 1 and b"n_partials" in err()
    assert moments(n_partials=257) == 1 and b"n_partials" in err()
    assert moments(elems=1) == 1 and b"sample_elems" in err()
    assert moments(elems=1 << 31) == 1 and moments(n_samples=0) == 1 and b"n_samples" in err()

    def call(W=128, x=X, out=OUT, out2=OUT2, x0_prev=H0, x0_out=H1, known=Z, noise=N, mask=M, rows=4, part=P, n_partials=64,
             sample_rows=2, phi=0.7, tstep=None, n_tstep=0):
        return lib.pf_cfg_rescaled_step_pair(x, EU, EC, 9.0, 0.5, 0.8, 0.6, 0.7, rows, W, 0, out, out2, tstep, n_tstep, 0,
                                             x0_prev, C.c_float(0.1), x0_out, known, noise, mask, C.c_float(0.6),
                                             C.c_float(0.7), 3, part, n_partials, sample_rows, C.c_float(phi), F, None)
    assert call(sample_rows=3) == 1 and b"sample_rows" in err()
    assert call(sample_rows=0) == 1 and b"sample_rows" in err()
    for phi in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(phi=phi) == 1 and b"phi" in err(), phi
    assert call(part=None) == 1 and b"partials" in err()
    assert call(n_partials=0) == 1 and b"n_partials" in err()
    assert call(n_partials=257) == 1 and b"n_partials" in err()
    # known / noise / mask: together or not at all
    for name in ("known", "noise", "mask"):
        assert call(**{name: None}) == 1 and b"together" in err(), name
        for alias in (OUT, OUT2, H1):
            assert call(**{name: alias}) == 1 and b"must not alias" in err(), (name, hex(alias))
    # everything the inpaint entry point refuses
    assert call(W=8193) == 1 and b"8192" in err()
    assert call(W=16385, x0_prev=None, x0_out=None) == 1 and b"16384" in err()
    assert call(x0_out=None) == 1 and b"x0_prev requires x0_out" in err()
    for alias in (X, EU, EC, OUT, OUT2):
        assert call(x0_out=alias) == 1, hex(alias)
    assert call(x0_prev=OUT) == 1 and call(x0_prev=OUT2) == 1
    assert call(out2=X) == 1 and call(out=EU) == 1
    assert call(rows=0) == 1 and call(W=0) == 1 and call(x=None) == 1 and call(out=None) == 1
    assert call(tstep=P, n_tstep=0) == 1 and b"n_tstep" in err()
    assert call(W=1, rows=4, sample_rows=1) == 1 and b"fewer than 2" in err()
