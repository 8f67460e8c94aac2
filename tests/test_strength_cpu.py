"""Strength < 1 sampling from a source panorama and DenoiseLoop.restart(), host side: the executed-step table
against a restatement of diffusers' get_timesteps, the start coefficients against fp32 add_noise, the 2M order sequence
against a restatement of DPMSolverMultistepScheduler.step's predicate, the loop on the test double tests/fake_ops.py against a
naive restatement (add_noise start, sliced timesteps, everything rolled with torch.roll), restart() against fresh loops (also
sharded over gloo), the ValueErrors, and the C entry point's argument checks (no launch, no GPU)."""
import ctypes as C
import math
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
from test_inpaint_cpu import _use_fake_backend as _inpaint_backend

HERE = os.path.dirname(os.path.abspath(__file__))
START_OP = {"enabled": False, "calls": []}


def noised_start_pair(z, noise, ka, kb, roll=0, *, out, out2=None, tstep=None, t0=0):
    """Torch stand-in for ops.noised_start_pair, set on the fake_ops module at run time.  It raises unless a test enabled it: a
    loop built with defaults must never get here."""
    if not START_OP["enabled"]:
        raise AssertionError("noised_start_pair called by a loop that must not use it")
    START_OP["calls"].append(dict(z=z, ka=ka, kb=kb, roll=roll, t0=t0, tstep=tstep is not None))
    y = torch.roll(noise.float() if z is None else ka * z + kb * noise, roll, -1)
    out.copy_(y)
    if out2 is not None:
        out2.copy_(y)
    if tstep is not None:
        tstep.fill_(int(t0))
    return out


def _use_fake_backend(put, extra=()):
    _inpaint_backend(put, extra)
    put(fake_ops, "noised_start_pair", noised_start_pair)


@pytest.fixture
def fake_backend(monkeypatch):
    _use_fake_backend(lambda o, n, v: monkeypatch.setattr(o, n, v, raising=False), ["panfusion_amd.sharding"])
    monkeypatch.setitem(START_OP, "enabled", False)
    monkeypatch.setitem(START_OP, "calls", [])
    return monkeypatch


@pytest.fixture
def start_op(fake_backend):
    fake_backend.setitem(START_OP, "enabled", True)
    return START_OP["calls"]


@pytest.fixture(scope="module")
def oracle_model():
    return build_tiny_oracle()


def _source(lat, pano, cams, seed=5):
    """Seeded source latents: _known's N(0, 1) panorama latent and its nearest e2p into the views."""
    from panfusion_amd.pipeline import SourceLatents
    k = _known(lat, pano, cams, seed=seed)
    return SourceLatents(k.latents, k.pano_latent)


def _zero_model(lat2, pano2, *a):
    return torch.zeros_like(lat2), torch.zeros_like(pano2)


# ------------------------------------------------------------------------------------------------- executed steps
def get_timesteps(timesteps, num_inference_steps, strength):
    """StableDiffusionImg2ImgPipeline.get_timesteps (diffusers 0.24), literally."""
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    return timesteps[t_start:], num_inference_steps - t_start


@pytest.mark.parametrize("n", [10, 20, 50])
def test_executed_steps_are_diffusers_get_timesteps(start_op, n):
    from oracle import ddim as oddim
    from panfusion_amd.pipeline import DenoiseLoop, executed_steps
    assert int(50 * 0.58) == 28                                   # Python's int() of the float product, quirks included
    lat, pano, pe, ppe, cams = _inputs()
    full = [int(t) for t in oddim.DDIM().set_timesteps(n)]
    for s in (0.05, 0.3, 0.5, 0.58, 0.6, 0.75, 0.99, 1.0):
        want, k = get_timesteps(full, n, s)
        build = lambda: DenoiseLoop(_zero_model, lat, pano, pe, ppe, cams, steps=n, strength=s, init=_source(lat, pano, cams))
        if k == 0:
            assert (n, s) == (10, 0.05)
            with pytest.raises(ValueError):
                build()
            with pytest.raises(ValueError):
                executed_steps(n, s)
            continue
        assert executed_steps(n, s) == (k, n - k)
        del start_op[:]
        loop = build()
        assert loop.timesteps == want and len(loop.timesteps) == k == min(int(n * s), n) and loop.i0 == n - k
        assert loop.timesteps == full[n - k:]
        if s < 1.0:
            assert [c["tstep"] for c in start_op] == [False, True] and start_op[1]["t0"] == want[0]     # views, then panorama
        else:
            assert start_op == []
        loop.run()
        assert loop.i == k and loop.total_rot == 90.0 * k
    assert executed_steps(10, 0.6) == (6, 4) and oddim.DDIM().set_timesteps(10)[4] == 501


@pytest.mark.parametrize("n", [10, 20, 50])
def test_start_coefficients_are_diffusers_add_noise(start_op, n):
    """DDIMSchedule.coefficients(t)[:2] = fp32 alphas_cumprod[t] ** 0.5, (1 - alphas_cumprod[t]) ** 0.5 (DDIMScheduler.add_noise)
    bit for bit at every t of the grid; the loop passes exactly that pair for its t_s to both start launches."""
    from oracle import ddim as oddim
    from panfusion_amd.pipeline import DDIMSchedule, DenoiseLoop
    ref = oddim.DDIM()
    ac = ref.alphas_cumprod
    assert ac.dtype == torch.float32
    sched = DDIMSchedule()
    assert torch.equal(sched.alphas_cumprod, ac)
    grid = sched.set_timesteps(n)
    assert grid == [int(t) for t in ref.set_timesteps(n)]
    for t in grid:
        assert sched.coefficients(t)[:2] == (float(ac[t] ** 0.5), float((1 - ac[t]) ** 0.5)), t
    lat, pano, pe, ppe, cams = _inputs()
    for i0 in (1, n // 2, n - 1):
        del start_op[:]
        DenoiseLoop(_zero_model, lat, pano, pe, ppe, cams, steps=n, strength=(n - i0 + 0.5) / n, init=_source(lat, pano, cams))
        t = grid[i0]
        assert [(c["ka"], c["kb"]) for c in start_op] == [(float(ac[t] ** 0.5), float((1 - ac[t]) ** 0.5))] * 2
        assert start_op[1]["t0"] == t


# ------------------------------------------------------------------------------------------------------ 2M order
def diffusers_orders(n, i0, solver_order=2, lower_order_final=True):
    """The order DPMSolverMultistepScheduler.step (0.24) picks at every executed step of a run that starts at grid index i0:
    step_index and len(self.timesteps) on the FULL grid (the pipelines slice a copy), lower_order_nums counting from the first
    executed step."""
    orders, lower_order_nums = [], 0
    for step_index in range(i0, n):
        final = (step_index == n - 1) and lower_order_final and n < 15
        if solver_order == 1 or lower_order_nums < 1 or final:
            orders.append(1)
        else:
            orders.append(2)
        if lower_order_nums < solver_order:
            lower_order_nums += 1
    return orders


@pytest.mark.parametrize("n,strength", [(10, 0.6), (20, 0.5), (50, 0.3)])
def test_2m_order_sequence_of_the_executed_steps(fake_backend, start_op, n, strength):
    from panfusion_amd.pipeline import DenoiseLoop
    from test_dpmpp_cpu import cfg_dpmpp_step_pair
    calls = []
    fake_backend.setattr(fake_ops, "cfg_dpmpp_step_pair", lambda *a, **kw: calls.append(kw) or cfg_dpmpp_step_pair(*a, **kw))
    lat, pano, pe, ppe, cams = _inputs()
    loop = DenoiseLoop(_zero_model, lat, pano, pe, ppe, cams, steps=n, strength=strength, sampler="dpmpp_2m",
                       init=_source(lat, pano, cams))
    loop.run()
    i0 = n - int(n * strength)
    want = diffusers_orders(n, i0)
    assert want[0] == 1 and want[1] == 2 and want[-1] == (1 if n < 15 else 2)
    got = [1 if kw["x0_prev"] is None else 2 for kw in calls]
    assert got[0::2] == want and got[1::2] == want
    for j, kw in enumerate(calls[0::2]):                       # a second-order step uses the full grid's coefficients unchanged
        coef, k, order = loop.solver.step_coefficients(i0 + j)
        if j > 0:
            assert order == want[j] and kw["k"] == k


# ------------------------------------------------------------------------------------------ the loop on the fake backend
def restated(model, n_v, n_p, pe, ppe, cams, z_v, z_p, known, steps, strength, sampler, rot_diff, guidance=9.0):
    """diffusers' img2img / inpaint pipelines around PanFusion.inference's loop (PanFusion.py:146-164) in fp32: add_noise start
    at the first sliced timestep, then per step the roll of the panorama -- and of its source, mask, noise and x0 history -- the
    CFG call, the DDIM or 2M update in diffusers' form and the 4-channel blend.  Returns ((start views, start panorama before the
    first roll), [(views, panorama in the state's own frame) after every step])."""
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
    roll = lambda t: torch.roll(t, shift, -1) if rot_diff % 360 else t
    latents, pano = (add_noise(z_v, n_v, ts[0]), add_noise(z_p, n_p, ts[0])) if strength < 1 else (n_v.clone(), n_p.clone())
    start = (latents, pano)
    if known is not None:
        m_v, m_p = known.mask, known.pano_mask
    else:
        m_v, m_p = torch.ones_like(n_v[:, :, :1]), torch.ones_like(n_p[:, :, :1])
    x0_v = x0_p = None
    traj = []
    m = latents.shape[1]
    for j, s0 in enumerate(ts):
        i = i0 + j
        pano, cams = oddim.rotate_latent(pano, cams, rot_diff)
        z_p, m_p, n_p = roll(z_p), roll(m_p), roll(n_p)
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
        for x, eps, x0_prev, z, mk, n in ((latents, oddim.cfg_merge(e, guidance), x0_v, z_v, m_v, n_v),
                                          (pano, oddim.cfg_merge(pe_, guidance), x0_p, z_p, m_p, n_p)):
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
    return start, traj


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("with_known", [False, True])
@pytest.mark.parametrize("rot_diff", [90.0, 37.0])
def test_strength_loop_matches_naive_restatement(start_op, oracle_model, sampler, with_known, rot_diff):
    """n = 10 at strength 0.6 (6 steps from t = 501; 2M ends first order, n < 15): the start state and the state after every
    step equal the restatement within 1e-4 rel-L2 -- the bound test_inpaint_cpu.test_loop_matches_naive_restatement uses for the
    same comparison.  With a known band the source is the known latents (init=None)."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    steps, strength = 10, 0.6
    lat, pano, pe, ppe, cams = _inputs()
    known = _known(lat, pano, cams) if with_known else None
    src = _source(lat, pano, cams)
    start, want = restated(oracle_model, lat, pano, pe, ppe, cams, src.latents, src.pano_latent, known, steps, strength,
                           sampler, rot_diff)
    loop = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=steps, rot_diff=rot_diff, sampler=sampler,
                       known=known, strength=strength, init=None if with_known else src)
    assert loop.timesteps[0] == 501 and len(loop.timesteps) == 6 == len(want)
    es = rel_l2(loop.lat, start[0]), rel_l2(torch.roll(loop.pano, -loop.shift, -1), start[1])
    assert max(es) < 1e-4, es
    assert torch.equal(loop.lat2[0], loop.lat2[1]) and torch.equal(loop.pano2[0], loop.pano2[1])
    assert torch.equal(loop.tstep, torch.full_like(loop.tstep, 501))
    for j in range(len(want)):
        loop.step()
        moved = 0 if j == len(want) - 1 else loop.shift
        ev, ep = rel_l2(loop.lat, want[j][0]), rel_l2(torch.roll(loop.pano, -moved, -1), want[j][1])
        assert ev < 1e-4 and ep < 1e-4, (sampler, with_known, rot_diff, j + 1, ev, ep)
    if with_known:                       # kept entries end on the known latents themselves (the panorama rolled 6 shifts)
        keep_v = known.mask.expand_as(lat) == 0
        assert torch.equal(loop.lat[keep_v], known.latents[keep_v])
        o = len(want) * loop.shift
        keep_p = torch.roll(known.pano_mask.expand_as(pano), o, -1) == 0
        assert torch.equal(loop.pano[keep_p], torch.roll(known.pano_latent, o, -1)[keep_p])
    # the feature is really in effect: the strength-1 loop differs after its first step
    full = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=steps, rot_diff=rot_diff, sampler=sampler,
                       known=known)
    full.step()
    assert rel_l2(full.lat, want[0][0]) > 1e-2


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_strength_one_ignores_init_and_defaults_never_call_the_start_op(fake_backend, oracle_model, sampler):
    """strength = 1.0 with init: the loop without init, bit for bit (is_strength_max), through today's set-up -- the stand-in of
    the new op is NOT enabled here and raises if called, also for the loops built with defaults."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    src = _source(lat, pano, cams)
    for known in (None, _known(lat, pano, cams)):
        a = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, sampler=sampler, known=known)
        b = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, sampler=sampler, known=known, strength=1.0,
                        init=src)
        assert a.timesteps == b.timesteps and b.i0 == 0
        for _ in range(3):
            a.step()
            b.step()
            assert torch.equal(a.lat2, b.lat2) and torch.equal(a.pano2, b.pano2) and torch.equal(a.tstep, b.tstep)
        assert all(torch.equal(x, y) for x, y in zip(a.result(), b.result()))
    assert START_OP["calls"] == []
    with pytest.raises(AssertionError):                          # and the stand-in does guard: a strength < 1 loop needs it
        DenoiseLoop(_zero_model, lat, pano, pe, ppe, cams, steps=10, strength=0.5, init=src)


# ------------------------------------------------------------------------------------------------------- restart()
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _noise(lat, pano, cams, seed):
    from oracle import ddim as oddim
    n_p = torch.randn(pano.shape, generator=torch.Generator().manual_seed(seed))
    return oddim.init_noise(n_p, cams, *lat.shape[-2:])[1], n_p


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("with_known", [False, True])
def test_restart_equals_a_fresh_loop(start_op, oracle_model, sampler, with_known):
    """Run 3 steps, restart, run to the end: bit-identical to a fresh loop -- with the same inputs, with new noise, a new source,
    a new strength (up and down, 1.0 included) and new known contents.  The state buffers keep their addresses."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    model = hip_model(oracle_model)
    known = _known(lat, pano, cams) if with_known else None
    src = _source(lat, pano, cams)
    make = lambda la=lat, pa=pano, **kw: DenoiseLoop(model, la, pa, pe, ppe, cams, steps=5, sampler=sampler,
                                                     **dict(dict(known=known, strength=0.8, init=src), **kw))
    loop = make()
    ptrs = [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep)]
    want = make().run()
    for _ in range(3):
        loop.step()
    loop.restart()
    assert loop.i == 0 and loop.total_rot == 90.0 and loop.timesteps == make().timesteps
    assert _same(loop.run(), want)
    loop.restart()                                           # after a full run too
    assert _same(loop.run(), want)
    n_v, n_p = _noise(lat, pano, cams, 21)
    loop.restart(n_v, n_p)
    assert _same(loop.run(), make(n_v, n_p).run())
    src2 = _source(lat, pano, cams, seed=6)
    loop.restart(init=src2)                                  # keeps the noise of the previous restart
    assert _same(loop.run(), make(n_v, n_p, init=src2).run())
    loop.restart(strength=0.4)
    assert len(loop.timesteps) == 2
    assert _same(loop.run(), make(n_v, n_p, init=src2, strength=0.4).run())
    loop.restart(lat, pano, strength=1.0)
    assert len(loop.timesteps) == 5 and loop.i0 == 0
    assert _same(loop.run(), make(strength=1.0, init=None).run())
    loop.restart(strength=0.6)                               # the source survives a strength-1 run
    assert _same(loop.run(), make(init=src2, strength=0.6).run())
    if with_known:
        k2 = _known(lat, pano, cams, soft=False, seed=9)
        loop.restart(known=k2, init=src)
        assert _same(loop.run(), make(known=k2, strength=0.6).run())
    assert ptrs == [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep)]


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_restart_of_a_loop_built_with_defaults(start_op, oracle_model, sampler):
    """"Next seed, same prompt": a plain text-to-panorama loop restarted with new noise equals a fresh loop on that noise; its
    construction did not use the start op, its restart does (z = None: the rolled noise)."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    model = hip_model(oracle_model)
    make = lambda la, pa, **kw: DenoiseLoop(model, la, pa, pe, ppe, cams, steps=3, sampler=sampler, **kw)
    loop = make(lat, pano)
    assert start_op == []
    first = [t.clone() for t in loop.run()]
    loop.restart()
    assert [c["z"] for c in start_op] == [None, None] and [c["roll"] for c in start_op] == [0, loop.shift]
    assert _same(loop.run(), first)
    n_v, n_p = _noise(lat, pano, cams, 22)
    loop.restart(n_v, n_p)
    assert _same(loop.run(), make(n_v, n_p).run())
    loop.restart(strength=0.7, init=_source(lat, pano, cams))
    assert _same(loop.run(), make(n_v, n_p, strength=0.7, init=_source(lat, pano, cams)).run())


# --------------------------------------------------------------------------------------- sharded loop over gloo
def _restart_scenario(make):
    """Build at strength 0.6 with known content, run one step, restart with new noise, a new source and strength 0.8, run."""
    lat, pano, pe, ppe, cams = args = _inputs()
    known = _known(lat, pano, cams)
    n_v, n_p = _noise(lat, pano, cams, 23)
    src = _source(lat, pano, cams, seed=7)
    loop = make(args, steps=5, sampler="dpmpp_2m", known=known, strength=0.6)
    loop.step()
    loop.restart(n_v, n_p, strength=0.8, init=src)
    restarted = [t.clone() for t in loop.run()]
    fresh = make((n_v, n_p, pe, ppe, cams), steps=5, sampler="dpmpp_2m", known=known, strength=0.8, init=src).run()
    return restarted, fresh


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
        torch.save(_restart_scenario(make), os.path.join(out, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_restart_equals_fresh_and_single_process(start_op):
    """World 2: every rank holds the full latents and operands, so a restarted sharded loop equals a fresh sharded loop bit for
    bit on every rank, the replicas stay bit-identical, and both equal the single-process loop."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    from test_sharding_gloo import _free_port
    world = 2
    model = hip_model(build_tiny_oracle())
    restarted, fresh = _restart_scenario(lambda args, **kw: DenoiseLoop(model, *args, **kw))
    assert _same(restarted, fresh)
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    for r_restarted, r_fresh in res:
        assert _same(r_restarted, r_fresh)
        assert rel_l2(r_restarted[0], fresh[0]) < 1e-4 and rel_l2(r_restarted[1], fresh[1]) < 1e-4
    assert _same(res[0][0], res[1][0])


# ---------------------------------------------------------------------------------------------------- bad inputs
def test_loop_and_restart_reject_bad_inputs(start_op):
    from panfusion_amd.pipeline import DenoiseLoop, SourceLatents
    lat, pano, pe, ppe, cams = _inputs()
    src, known = _source(lat, pano, cams), _known(lat, pano, cams)
    loop = lambda la=lat, pa=pano, **kw: DenoiseLoop(None, la, pa, pe, ppe, cams, steps=10, **kw)
    two = lambda t: torch.cat([t, t])
    for s in (0.0, -0.3, 1.0001, 2, float("nan"), float("inf"), 0.05, None, "0.5"):
        with pytest.raises(ValueError):
            loop(strength=s, init=src)
    with pytest.raises(ValueError):
        loop(strength=0.5)                                        # neither init nor known
    bad = [SourceLatents(src.latents[..., :8], src.pano_latent), SourceLatents(src.latents, src.pano_latent[..., :16]),
           SourceLatents(src.latents[:, :3], src.pano_latent), SourceLatents(None, src.pano_latent),
           SourceLatents(two(src.latents), two(src.pano_latent))]
    for init in bad:
        with pytest.raises(ValueError):
            loop(strength=0.5, init=init)
        with pytest.raises(ValueError):
            loop(strength=1.0, init=init)                         # checked at strength 1 too
    with pytest.raises(ValueError):
        loop(two(lat), two(pano), strength=0.5, init=SourceLatents(two(src.latents), two(src.pano_latent)))
    assert len(loop(strength=0.5, init=src).timesteps) == 5 and len(loop(strength=0.5, known=known).timesteps) == 5
    # restart
    plain, img, kn = loop(), loop(strength=0.5, init=src), loop(strength=0.5, known=known)
    for lp in (plain, img, kn):
        for kw in (dict(strength=0.0), dict(strength=float("nan")), dict(strength=0.05), dict(strength=1.5),
                   dict(latents=lat[..., :8]), dict(pano_latent=two(pano)), dict(latents=two(lat), pano_latent=two(pano)),
                   dict(init=bad[0]), dict(init=bad[4])):
            with pytest.raises(ValueError):
                lp.restart(**kw)
    with pytest.raises(ValueError):
        plain.restart(known=known)                                # built without known content
    with pytest.raises(ValueError):
        img.restart(known=known)
    with pytest.raises(ValueError):
        plain.restart(strength=0.5)                               # no source
    with pytest.raises(ValueError):
        kn.restart(known=type(known)(known.latents, known.mask * 1.5, known.pano_latent, known.pano_mask))
    # a refused restart leaves the loop as it was
    assert img.strength == 0.5 and len(img.timesteps) == 5 and plain.strength == 1.0 and plain.src_lat is None
    kn.restart(known=known, strength=0.7)
    assert len(kn.timesteps) == 7


# ------------------------------------------------------------------------------------- C entry point: argument checks
def test_entry_point_rejects_bad_arguments_before_launching():
    """Validation happens before any launch (fake, never dereferenced device addresses; every call below must fail)."""
    from panfusion_amd import _lib
    lib = _lib.lib()
    Z, N, OUT, OUT2, T = (0x10000 * i for i in range(1, 6))

    def call(z=Z, noise=N, rows=4, W=128, out=OUT, out2=OUT2, tstep=None, n_tstep=0):
        return lib.pf_noised_start_pair(z, noise, C.c_float(0.6), C.c_float(0.8), rows, W, 3, out, out2, tstep, n_tstep, 501, None)
    assert call(noise=None) == 1 and b"pf_noised_start_pair" in lib.pf_last_error_string()
    assert call(out=None) == 1
    assert call(out2=OUT) == 1 and b"out2" in lib.pf_last_error_string()
    assert call(out=Z) == 1 and b"alias" in lib.pf_last_error_string()
    assert call(out2=Z) == 1 and call(out=N) == 1 and call(out2=N) == 1
    assert call(W=16385) == 1 and b"16384" in lib.pf_last_error_string()
    assert call(tstep=T, n_tstep=0) == 1 and b"n_tstep" in lib.pf_last_error_string()
    assert call(rows=0) == 1 and call(W=0) == 1 and call(rows=1 << 31) == 1
    assert call(z=None, noise=None) == 1
    assert math.isfinite(lib.pf_version())
