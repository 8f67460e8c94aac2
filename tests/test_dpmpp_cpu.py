"""DPM-Solver++(2M) sampler, host side: the schedule against diffusers' published update (restated here in float64), the
loop logic on the test double tests/fake_ops.py (history roll, order switch, un-roll in result()), the sharded loop over
gloo, and the C entry point's argument checks (no launch, no GPU)."""
import ctypes as C
import importlib
import math
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fake_ops
from conftest import build_tiny_oracle, cam4, golden, rel_l2

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------------- test 1: schedule
def _alpha_sigma(ac, t):
    a = float(ac[t] if t >= 0 else ac[0])
    return math.sqrt(a), math.sqrt(1.0 - a)


def diffusers_2m(sched, n, x, eps, x0_prev, i, order):
    """One step of diffusers' DPMSolverMultistepScheduler (dpmsolver++, midpoint) in its own form, float64 tensors:
    dpm_solver_first_order_update / multistep_dpm_solver_second_order_update on DDIMSchedule's grid."""
    ac = sched.alphas_cumprod
    ts = sched.timesteps
    s0 = ts[i]
    t = s0 - 1000 // n
    alpha_s0, sigma_s0 = (torch.tensor(v, dtype=torch.float64) for v in _alpha_sigma(ac, s0))
    alpha_t, sigma_t = (torch.tensor(v, dtype=torch.float64) for v in _alpha_sigma(ac, t))
    lam = lambda a, s: torch.log(a) - torch.log(s)
    x0 = (x - sigma_s0 * eps) / alpha_s0
    h = lam(alpha_t, sigma_t) - lam(alpha_s0, sigma_s0)
    if order == 1:
        return (sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * x0, x0
    alpha_s1, sigma_s1 = (torch.tensor(v, dtype=torch.float64) for v in _alpha_sigma(ac, ts[i - 1]))
    r0 = (lam(alpha_s0, sigma_s0) - lam(alpha_s1, sigma_s1)) / h
    D0, D1 = x0, (1.0 / r0) * (x0 - x0_prev)
    return ((sigma_t / sigma_s0) * x - (alpha_t * (torch.exp(-h) - 1.0)) * D0
            - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1), x0


@pytest.mark.parametrize("n", [10, 20, 25, 50])
def test_schedule_grid_and_ddim_plus_correction_equals_diffusers_form(n):
    from panfusion_amd.pipeline import DDIMSchedule, DPMSolverSchedule
    ddim, sched = DDIMSchedule(), DPMSolverSchedule()
    assert sched.set_timesteps(n) == ddim.set_timesteps(n)
    assert torch.equal(sched.alphas_cumprod, ddim.alphas_cumprod)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(3, 4, 8, 16, generator=g, dtype=torch.float64)
    ours = ref = x
    x0_ours = x0_ref = None
    for i, s0 in enumerate(sched.timesteps):
        coef, k, order = sched.step_coefficients(i)
        assert coef == ddim.coefficients(s0)                          # the DDIM part: DDIMSchedule's fp32 values, bit for bit
        eps = torch.randn(3, 4, 8, 16, generator=g, dtype=torch.float64)
        # the kernel's form, in float64: DDIM(x, eps) + k (x0 - x0_prev), DDIM on the float64 alpha / sigma of the definition
        a_s, s_s = _alpha_sigma(sched.alphas_cumprod, s0)
        a_t, s_t = _alpha_sigma(sched.alphas_cumprod, s0 - 1000 // n)
        x0 = (ours - s_s * eps) / a_s
        ddim_x = a_t * x0 + s_t * eps
        ours = ddim_x if order == 1 else ddim_x + k * (x0 - x0_ours)
        x0_ours = x0
        ref, x0_ref = diffusers_2m(sched, n, ref, eps, x0_ref, i, order)
        assert rel_l2(ours, ref) <= 1e-12, (n, i, order, rel_l2(ours, ref))
        if order == 1:
            assert k == 0.0


def test_order_pattern():
    from panfusion_amd.pipeline import DPMSolverSchedule
    for n in (1, 2, 4, 10, 14, 15, 20, 25, 50):
        s = DPMSolverSchedule()
        s.set_timesteps(n)
        want = [1] + [2] * (n - 1)
        if n < 15:
            want[-1] = 1                                                # lower_order_final
        assert [s.order(i) for i in range(n)] == want, n
        assert [s.step_coefficients(i)[2] for i in range(n)] == want
    s = DPMSolverSchedule(lower_order_final=False)
    s.set_timesteps(10)
    assert [s.order(i) for i in range(10)] == [1] + [2] * 9
    s = DPMSolverSchedule(solver_order=1)
    s.set_timesteps(20)
    assert all(s.step_coefficients(i)[1:] == (0.0, 1) for i in range(20))
    with pytest.raises(ValueError):
        DPMSolverSchedule(solver_order=3)


# ------------------------------------------------------------------------------------------ test 2: loop on the fake backend
def cfg_dpmpp_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                        x0_prev=None, k=0.0, x0_out=None):
    """Torch stand-in for ops.cfg_dpmpp_step_pair, set on the fake_ops module at run time (the order-1 path is fake_ops'
    cfg_ddim_step arithmetic, so an order-1 loop equals the DDIM loop bit for bit)."""
    sa, sb, sap, sbp = coef
    eps = eps_uncond + guidance * (eps_cond - eps_uncond)
    x0 = (x - sb * eps) / sa
    y = sap * x0 + sbp * eps
    if x0_prev is not None:
        y = y + k * (x0 - x0_prev)
    y, x0 = torch.roll(y, roll, -1), torch.roll(x0, roll, -1)
    out = y if out is None else out.copy_(y)
    if out2 is not None:
        out2.copy_(y)
    x0_out = x0 if x0_out is None else x0_out.copy_(x0)
    if tstep is not None:
        tstep.fill_(int(t_next))
    return out, x0_out


def _use_fake_backend(put, extra=()):
    """put(obj, name, value): monkeypatch.setattr in this process, plain setattr in a spawned worker."""
    from test_engine_logic_cpu import MODS
    for name in list(MODS) + list(extra):
        put(importlib.import_module(name), "ops", fake_ops)
    put(fake_ops, "cfg_dpmpp_step_pair", cfg_dpmpp_step_pair)


@pytest.fixture
def fake_backend(monkeypatch):
    _use_fake_backend(lambda o, n, v: monkeypatch.setattr(o, n, v, raising=False), ["panfusion_amd.sharding"])
    return monkeypatch


@pytest.fixture(scope="module")
def oracle_model():
    return build_tiny_oracle()


def _inputs():
    g = golden("mvgen_tiny.npz")
    t = lambda k: torch.from_numpy(g[k])
    cam1 = {k: v[None] for k, v in cam4().items()}
    return t("latents")[:1], t("pano_latent")[:1], t("prompt_embd"), t("pano_prompt_embd"), cam1


def restated_2m(model, latents, pano, pe, ppe, cams, steps, rot_diff=90.0, guidance=9.0):
    """PanFusion.inference's loop (PanFusion.py:146-164) with diffusers' 2M update in fp32 (tools/make_golden_dpmpp.py's
    form): the panorama and its x0 history are rolled before every call, the rotation undone at the end.  Returns the
    (views, un-rotated panorama) after every step."""
    from oracle import ddim as oddim
    ac = oddim.DDIM().alphas_cumprod
    ts = [int(t) for t in oddim.DDIM().set_timesteps(steps)]
    a_s = lambda t: ((ac[t] if t >= 0 else ac[0]) ** 0.5, (1 - (ac[t] if t >= 0 else ac[0])) ** 0.5)
    lam = lambda t: torch.log(a_s(t)[0]) - torch.log(a_s(t)[1])
    x0_v = x0_p = None
    total, traj = 0.0, []
    m = latents.shape[1]
    for i, s0 in enumerate(ts):
        pano, cams = oddim.rotate_latent(pano, cams, rot_diff)
        if x0_p is not None:
            x0_p = torch.roll(x0_p, int(rot_diff / 360 * pano.shape[-1]), -1)
        total += rot_diff
        with torch.no_grad():
            e, pe_ = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano), torch.full((2, m), s0, dtype=torch.long), pe, ppe,
                           oddim.cfg_pair(cams))
        t = s0 - 1000 // steps
        (al_s, sg_s), (al_t, sg_t) = a_s(s0), a_s(t)
        h = lam(t) - lam(s0)
        second = 0 < i and not (i == steps - 1 and steps < 15)
        new = []
        for x, eps, x0_prev in ((latents, oddim.cfg_merge(e, guidance), x0_v), (pano, oddim.cfg_merge(pe_, guidance), x0_p)):
            x0 = (x - sg_s * eps) / al_s
            y = (sg_t / sg_s) * x - (al_t * (torch.exp(-h) - 1.0)) * x0
            if second:
                r0 = (lam(s0) - lam(ts[i - 1])) / h
                y = y - 0.5 * (al_t * (torch.exp(-h) - 1.0)) * ((1.0 / r0) * (x0 - x0_prev))
            new.append((y, x0))
        (latents, x0_v), (pano, x0_p) = new
        traj.append((latents, torch.roll(pano, int(-total / 360 * pano.shape[-1]), -1)))
    return traj


def test_loop_2m_matches_restatement(fake_backend, oracle_model):
    """Four steps (orders 1, 2, 2, 1): the history is rolled with the panorama, the order switches where the schedule says,
    result() undoes the rotation; the loop on the fake backend equals the restatement driven by the CPU oracle."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    calls = []

    def spy(*a, **kw):
        calls.append((kw.get("x0_prev") is not None, kw.get("k", 0.0)))
        return cfg_dpmpp_step_pair(*a, **kw)
    fake_backend.setattr(fake_ops, "cfg_dpmpp_step_pair", spy)
    steps = 4
    args = _inputs()
    want = restated_2m(oracle_model, *args, steps)
    loop = DenoiseLoop(hip_model(oracle_model), *args, steps=steps, sampler="dpmpp_2m")
    for i in range(steps):
        loop.step()
        pano = torch.roll(loop.pano, int(-loop.total_rot / 360 * loop.W), -1)
        ev, ep = rel_l2(loop.lat, want[i][0]), rel_l2(pano, want[i][1])
        assert ev < 1e-4 and ep < 1e-4, (i + 1, ev, ep)
    lat, pano = loop.result()
    assert rel_l2(lat, want[-1][0]) < 1e-4 and rel_l2(pano, want[-1][1]) < 1e-4
    # two launches per step; second order at steps 2 and 3 only, with k > 0
    assert [c[0] for c in calls] == [False, False, True, True, True, True, False, False]
    assert all(k > 0 for second, k in calls if second)
    # the multistep correction is really there: DDIM agrees with 2M after the first (first-order) step and not after the second
    ddim = DenoiseLoop(hip_model(oracle_model), *args, steps=steps)
    ddim.step()
    assert rel_l2(ddim.lat, want[0][0]) < 1e-4
    ddim.step()
    assert rel_l2(ddim.lat, want[1][0]) > 1e-3


def test_order_one_loop_is_the_ddim_loop(fake_backend, oracle_model):
    from panfusion_amd.pipeline import DenoiseLoop, DPMSolverSchedule
    from test_engine_logic_cpu import hip_model
    args = _inputs()
    a = DenoiseLoop(hip_model(oracle_model), *args, steps=3)
    b = DenoiseLoop(hip_model(oracle_model), *args, steps=3, sampler=DPMSolverSchedule(solver_order=1))
    for _ in range(3):
        a.step()
        b.step()
        assert torch.equal(a.lat2, b.lat2) and torch.equal(a.pano2, b.pano2) and torch.equal(a.tstep, b.tstep)
    assert all(torch.equal(x, y) for x, y in zip(a.result(), b.result()))


def test_sampler_argument(fake_backend):
    from panfusion_amd.pipeline import DenoiseLoop, DPMSolverSchedule
    z = (torch.zeros(1, 4, 4, 4, 4), torch.zeros(1, 1, 4, 4, 8), torch.zeros(2, 4, 3, 8), torch.zeros(2, 1, 3, 8),
         {k: v[None] for k, v in cam4().items()})
    for bad in ("euler", "DDIM", "dpmpp_3m", None, 2):
        with pytest.raises(ValueError):
            DenoiseLoop(None, *z, steps=4, sampler=bad)
    assert DenoiseLoop(None, *z, steps=4).solver is None
    loop = DenoiseLoop(None, *z, steps=4, sampler="dpmpp_2m")
    assert loop.solver.solver_order == 2 and loop.solver.timesteps == loop.timesteps
    assert loop.x0_lat.shape == (1, 4, 4, 4, 4) and loop.x0_pano.shape == (1, 1, 4, 4, 8)
    assert loop.x0_lat.dtype == loop.x0_pano.dtype == torch.float32
    mine = DPMSolverSchedule(solver_order=1)
    mine.set_timesteps(7)
    loop = DenoiseLoop(None, *z, steps=4, sampler=mine)
    assert loop.solver is not mine and loop.solver.solver_order == 1 and len(loop.solver.timesteps) == 4
    assert len(mine.timesteps) == 7                                          # the caller's object is left alone


# --------------------------------------------------------------------------------------- test 3: sharded loop over gloo
def _run_loop(sharded, steps):
    from panfusion_amd import sharding
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    model = hip_model(build_tiny_oracle())
    args = _inputs()
    if sharded:
        loop = sharding.ShardedDenoiseLoop(model, sharding.make_shard(4), *args, steps=steps, sampler="dpmpp_2m")
    else:
        loop = DenoiseLoop(model, *args, steps=steps, sampler="dpmpp_2m")
    assert loop.solver is not None
    return loop.run()


def _worker(rank, world, port, out, steps):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    _use_fake_backend(setattr, ["panfusion_amd.sharding"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_run_loop(True, steps), os.path.join(out, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_2m_loop_equals_single_process(world, fake_backend):
    """Every rank keeps its own x0 history, computed from the same gathered epsilons: the replicas stay bit-identical and equal
    the single-process loop (three steps: orders 1, 2, 1 -- the second-order step reads the rolled panorama history)."""
    from test_sharding_gloo import _free_port
    steps = 3
    want = _run_loop(False, steps)
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(world, _free_port(), out, steps), nprocs=world, join=True)
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    for lat, pano in res:
        assert rel_l2(lat, want[0]) < 1e-4 and rel_l2(pano, want[1]) < 1e-4, (rel_l2(lat, want[0]), rel_l2(pano, want[1]))
    assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])


# ------------------------------------------------------------------------------------- C entry point: argument checks
def test_entry_point_rejects_bad_arguments_before_launching():
    """Validation happens before any launch (fake, never dereferenced device addresses): W > 8192 (two staged rows = 64 KB of
    LDS), x0_out missing or aliasing the state / predictions, x0_prev aliasing the state."""
    from panfusion_amd import _lib
    lib = _lib.lib()
    X, EU, EC, OUT, OUT2, H0, H1 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000

    def call(W=128, x=X, out=OUT, out2=OUT2, x0_prev=H0, x0_out=H1, rows=4):
        return lib.pf_cfg_dpmpp_step_pair(x, EU, EC, 9.0, 0.5, 0.8, 0.6, 0.7, rows, W, 0, out, out2, None, 0, 0,
                                          x0_prev, C.c_float(0.1), x0_out, None)
    assert call(W=8193) == 1 and b"8192" in lib.pf_last_error_string()
    assert call(x0_out=None) == 1
    for alias in (X, EU, EC, OUT, OUT2):
        assert call(x0_out=alias) == 1, hex(alias)
    assert call(x0_prev=OUT) == 1 and call(x0_prev=OUT2) == 1
    assert call(out2=X) == 1 and call(out=EU) == 1
    assert call(rows=0) == 1
