"""Known-region sampling (inpainting / outpainting), host side: the blend coefficients against diffusers' add_noise, the loop
logic on the test double tests/fake_ops.py against a naive restatement (the panorama's known latent, mask and noise rolled with
torch.roll together with the state), mask = 1 against the loop without known content, the sharded loop over gloo, the C entry
point's argument checks (no launch, no GPU) and DenoiseLoop's checks of the known inputs."""
import ctypes as C
import importlib
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import fake_ops
from conftest import build_tiny_oracle, cam4, golden, rel_l2
from test_dpmpp_cpu import cfg_dpmpp_step_pair

HERE = os.path.dirname(os.path.abspath(__file__))


def cfg_inpaint_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                          x0_prev=None, k=0.0, x0_out=None, *, known, noise, mask, ka, kb, known_roll=0):
    """Torch stand-in for ops.cfg_inpaint_step_pair, set on the fake_ops module at run time: fake_ops' DDIM arithmetic (plus the
    2M correction with x0_out), then m v + (1 - m) (ka known + kb noise) with the operands read at (w - known_roll) mod W."""
    sa, sb, sap, sbp = coef
    eps = eps_uncond + guidance * (eps_cond - eps_uncond)
    x0 = (x - sb * eps) / sa
    y = sap * x0 + sbp * eps
    if x0_prev is not None:
        y = y + k * (x0 - x0_prev)
    z, n, m = (torch.roll(t, known_roll, -1) for t in (known, noise, mask))
    y = torch.roll(m * y + (1 - m) * (ka * z + kb * n), roll, -1)
    out = y if out is None else out.copy_(y)
    if out2 is not None:
        out2.copy_(y)
    if x0_out is not None:
        x0_out.copy_(torch.roll(x0, roll, -1))
    if tstep is not None:
        tstep.fill_(int(t_next))
    return out, x0_out


def _use_fake_backend(put, extra=()):
    """put(obj, name, value): monkeypatch.setattr in this process, plain setattr in a spawned worker."""
    from test_engine_logic_cpu import MODS
    for name in list(MODS) + list(extra):
        put(importlib.import_module(name), "ops", fake_ops)
    put(fake_ops, "cfg_dpmpp_step_pair", cfg_dpmpp_step_pair)
    put(fake_ops, "cfg_inpaint_step_pair", cfg_inpaint_step_pair)


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


def _known(latents, pano, cams, soft=True, seed=5):
    """Seeded known content for the tiny loop: a N(0, 1) panorama latent kept on a band across the seam ([W - 4, W) and [0, 10)),
    with a soft band (m = 0.3) in the middle; the views' content and masks are the nearest e2p of the panorama's (init_noise)."""
    from oracle import ddim as oddim
    from panfusion_amd.pipeline import KnownRegion
    W = pano.shape[-1]
    z = torch.randn(pano.shape, generator=torch.Generator().manual_seed(seed))
    mask = torch.ones(1, 1, 1, *pano.shape[-2:])
    mask[..., W - 4:] = 0.0
    mask[..., :10] = 0.0
    if soft:
        mask[..., 14:18] = 0.3
    h, w = latents.shape[-2:]
    _, z_v = oddim.init_noise(z, cams, h, w)
    _, m_v = oddim.init_noise(mask, cams, h, w)
    return KnownRegion(z_v, m_v, z, mask)


# -------------------------------------------------------------------------------------------- blend coefficients
def _spy_loop(monkeypatch, sampler, steps, known=True):
    """A loop whose denoiser returns zeros, with every call of the new op recorded."""
    from panfusion_amd.pipeline import DenoiseLoop
    calls = []

    def spy(*a, **kw):
        calls.append(kw)
        return cfg_inpaint_step_pair(*a, **kw)
    monkeypatch.setattr(fake_ops, "cfg_inpaint_step_pair", spy)
    lat, pano, pe, ppe, cams = _inputs()
    model = lambda lat2, pano2, *a: (torch.zeros_like(lat2), torch.zeros_like(pano2))
    loop = DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=steps, sampler=sampler,
                       known=_known(lat, pano, cams) if known else None)
    loop.run()
    return loop, calls


@pytest.mark.parametrize("n", [10, 20, 50])
def test_blend_coefficients_are_diffusers_add_noise_at_the_next_timestep(fake_backend, n):
    """(ka, kb) of step i = diffusers DDIMScheduler.add_noise's sqrt(abar) / sqrt(1 - abar) at timesteps[i + 1] (fp32, bit for
    bit), (1, 0) at the last step (init_latents_proper = image_latents); both launches of a step use the same pair."""
    from oracle import ddim as oddim
    sched = oddim.DDIM()
    ts = [int(t) for t in sched.set_timesteps(n)]
    for sampler in ("ddim", "dpmpp_2m"):
        loop, calls = _spy_loop(fake_backend, sampler, n)
        assert len(calls) == 2 * n
        for i in range(n):
            a = sched.alphas_cumprod[ts[i + 1]] if i < n - 1 else None
            want = (float(a ** 0.5), float((1 - a) ** 0.5)) if a is not None else (1.0, 0.0)
            for kw in calls[2 * i:2 * i + 2]:
                assert (kw["ka"], kw["kb"]) == want, (sampler, i)


def test_known_roll_is_the_sum_of_the_shifts(fake_backend):
    """The views' operands are read in place, the panorama's at (i + 1) shift mod W -- also where rot_diff does not divide 360."""
    from panfusion_amd.pipeline import DenoiseLoop
    lat, pano, pe, ppe, cams = _inputs()
    W = pano.shape[-1]
    for rot in (90.0, 37.0, -50.0):
        calls = []
        fake_backend.setattr(fake_ops, "cfg_inpaint_step_pair", lambda *a, **kw: calls.append(kw) or cfg_inpaint_step_pair(*a, **kw))
        model = lambda lat2, pano2, *a: (torch.zeros_like(lat2), torch.zeros_like(pano2))
        DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=6, rot_diff=rot, known=_known(lat, pano, cams)).run()
        shift = int(rot / 360 * W)
        assert [kw["known_roll"] for kw in calls[0::2]] == [0] * 6
        assert [kw["known_roll"] for kw in calls[1::2]] == [(i + 1) * shift % W for i in range(6)], rot


# ------------------------------------------------------------------------------------------ the loop on the fake backend
def restated(model, latents, pano, pe, ppe, cams, known, steps, sampler, rot_diff, guidance=9.0):
    """PanFusion.inference's loop (PanFusion.py:146-164) with diffusers' update (DDIM, or 2M in its own form as in
    test_dpmpp_cpu.restated_2m) and StableDiffusionInpaintPipeline's 4-channel blend in fp32 -- the panorama's known latent,
    mask, noise and x0 history rolled with torch.roll together with the latent before every call.  Returns the (views,
    panorama in the state's own frame) after every step."""
    from oracle import ddim as oddim
    ddim = oddim.DDIM()
    ac = ddim.alphas_cumprod
    ts = [int(t) for t in ddim.set_timesteps(steps)]
    a_s = lambda t: ((ac[t] if t >= 0 else ac[0]) ** 0.5, (1 - (ac[t] if t >= 0 else ac[0])) ** 0.5)
    lam = lambda t: torch.log(a_s(t)[0]) - torch.log(a_s(t)[1])
    shift = int(rot_diff / 360 * pano.shape[-1])
    roll = lambda t: torch.roll(t, shift, -1) if rot_diff % 360 else t
    z_v, m_v, z_p, m_p = known.latents, known.mask, known.pano_latent, known.pano_mask
    n_v, n_p = latents.clone(), pano.clone()
    x0_v = x0_p = None
    traj = []
    m = latents.shape[1]
    for i, s0 in enumerate(ts):
        pano, cams = oddim.rotate_latent(pano, cams, rot_diff)
        z_p, m_p, n_p = roll(z_p), roll(m_p), roll(n_p)
        x0_p = None if x0_p is None else roll(x0_p)
        with torch.no_grad():
            e, pe_ = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano), torch.full((2, m), s0, dtype=torch.long), pe, ppe,
                           oddim.cfg_pair(cams))
        t = s0 - 1000 // steps
        (al_s, sg_s), (al_t, sg_t) = a_s(s0), a_s(t)
        h = lam(t) - lam(s0)
        second = sampler == "dpmpp_2m" and 0 < i and not (i == steps - 1 and steps < 15)
        last = i == steps - 1
        new = []
        for x, eps, x0_prev, z, mk, n in ((latents, oddim.cfg_merge(e, guidance), x0_v, z_v, m_v, n_v),
                                          (pano, oddim.cfg_merge(pe_, guidance), x0_p, z_p, m_p, n_p)):
            if sampler == "ddim":
                y, x0 = ddim.step(eps, s0, x), None
            else:
                x0 = (x - sg_s * eps) / al_s
                y = (sg_t / sg_s) * x - (al_t * (torch.exp(-h) - 1.0)) * x0
                if second:
                    r0 = (lam(s0) - lam(ts[i - 1])) / h
                    y = y - 0.5 * (al_t * (torch.exp(-h) - 1.0)) * ((1.0 / r0) * (x0 - x0_prev))
            proper = z if last else ac[ts[i + 1]] ** 0.5 * z + (1 - ac[ts[i + 1]]) ** 0.5 * n      # scheduler.add_noise
            new.append(((1 - mk) * proper + mk * y, x0))
        (latents, x0_v), (pano, x0_p) = new
        traj.append((latents, pano))
    return traj


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("rot_diff", [90.0, 37.0])
def test_loop_matches_naive_restatement(fake_backend, oracle_model, sampler, rot_diff):
    """Four steps: the loop (operands in the caller's frame, read at the offset) equals the restatement (operands rolled with the
    state) after every step; the loop's panorama is compared in the state's own frame, which the next roll has already moved."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    steps = 4
    lat, pano, pe, ppe, cams = _inputs()
    known = _known(lat, pano, cams)
    want = restated(oracle_model, lat, pano, pe, ppe, cams, known, steps, sampler, rot_diff)
    loop = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=steps, rot_diff=rot_diff, sampler=sampler,
                       known=known)
    for i in range(steps):
        loop.step()
        moved = 0 if i == steps - 1 else loop.shift
        ev, ep = rel_l2(loop.lat, want[i][0]), rel_l2(torch.roll(loop.pano, -moved, -1), want[i][1])
        assert ev < 1e-4 and ep < 1e-4, (sampler, rot_diff, i + 1, ev, ep)
    # the kept entries are the known latents themselves at the end (the panorama's in the state's frame, rolled (N) shifts)
    keep_v = known.mask.expand_as(lat) == 0
    assert torch.equal(loop.lat[keep_v], known.latents[keep_v])
    o = steps * loop.shift
    keep_p = torch.roll(known.pano_mask.expand_as(pano), o, -1) == 0
    assert torch.equal(loop.pano[keep_p], torch.roll(known.pano_latent, o, -1)[keep_p])
    # the blend is really there: without known content the loop differs after the first step
    free = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=steps, rot_diff=rot_diff, sampler=sampler)
    free.step()
    assert rel_l2(free.lat, want[0][0]) > 1e-2


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_mask_one_is_the_plain_loop(fake_backend, oracle_model, sampler):
    """m = 1 everywhere: the state (both halves of the pair), the timestep words and the 2M history after every step are the
    known=None loop's, bit for bit."""
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    k = _known(lat, pano, cams)
    ones = KnownRegion(k.latents, torch.ones_like(k.mask), k.pano_latent, torch.ones_like(k.pano_mask))
    a = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, sampler=sampler)
    b = DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=3, sampler=sampler, known=ones)
    for _ in range(3):
        a.step()
        b.step()
        assert torch.equal(a.lat2, b.lat2) and torch.equal(a.pano2, b.pano2) and torch.equal(a.tstep, b.tstep)
        if sampler != "ddim":
            assert torch.equal(a.x0_lat, b.x0_lat) and torch.equal(a.x0_pano, b.x0_pano)
    assert all(torch.equal(x, y) for x, y in zip(a.result(), b.result()))


def test_without_known_the_new_op_is_never_called(fake_backend):
    for sampler in ("ddim", "dpmpp_2m"):
        loop, calls = _spy_loop(fake_backend, sampler, 4, known=False)
        assert calls == [] and loop.known is None
        loop, calls = _spy_loop(fake_backend, sampler, 4, known=True)
        assert len(calls) == 8


# --------------------------------------------------------------------------------------- sharded loop over gloo
def _run_loop(sharded, steps, sampler):
    from panfusion_amd import sharding
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    model = hip_model(build_tiny_oracle())
    lat, pano, pe, ppe, cams = args = _inputs()
    known = _known(lat, pano, cams)
    if sharded:
        loop = sharding.ShardedDenoiseLoop(model, sharding.make_shard(4), *args, steps=steps, sampler=sampler, known=known)
    else:
        loop = DenoiseLoop(model, *args, steps=steps, sampler=sampler, known=known)
    return loop.run()


def _worker(rank, world, port, out, steps, sampler):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    _use_fake_backend(setattr, ["panfusion_amd.sharding"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_run_loop(True, steps, sampler), os.path.join(out, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_known_loop_equals_single_process(world, fake_backend):
    """Every rank holds the full latents and the known operands and blends after the same gathered epsilons: the replicas stay
    bit-identical and equal the single-process loop (three steps of 2M, known content across the seam)."""
    from test_sharding_gloo import _free_port
    steps, sampler = 3, "dpmpp_2m"
    want = _run_loop(False, steps, sampler)
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(world, _free_port(), out, steps, sampler), nprocs=world, join=True)
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    for lat, pano in res:
        assert rel_l2(lat, want[0]) < 1e-4 and rel_l2(pano, want[1]) < 1e-4, (rel_l2(lat, want[0]), rel_l2(pano, want[1]))
    assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])


# ------------------------------------------------------------------------------------- C entry point: argument checks
def test_entry_point_rejects_bad_arguments_before_launching():
    """Validation happens before any launch (fake, never dereferenced device addresses; every call below must fail): missing
    known / noise / mask, an operand aliasing out / out2 / x0_out, x0_prev without x0_out, the W limits of the two forms."""
    from panfusion_amd import _lib
    lib = _lib.lib()
    X, EU, EC, OUT, OUT2, H0, H1, Z, N, M = (0x10000 * i for i in range(1, 11))

    def call(W=128, x=X, out=OUT, out2=OUT2, x0_prev=H0, x0_out=H1, known=Z, noise=N, mask=M, rows=4):
        return lib.pf_cfg_inpaint_step_pair(x, EU, EC, 9.0, 0.5, 0.8, 0.6, 0.7, rows, W, 0, out, out2, None, 0, 0,
                                            x0_prev, C.c_float(0.1), x0_out, known, noise, mask, C.c_float(0.6),
                                            C.c_float(0.7), 3, None)
    assert call(W=8193) == 1 and b"8192" in lib.pf_last_error_string()
    assert call(W=16385, x0_prev=None, x0_out=None) == 1 and b"16384" in lib.pf_last_error_string()
    assert call(x0_out=None) == 1 and b"x0_prev requires x0_out" in lib.pf_last_error_string()
    for name in ("known", "noise", "mask"):
        assert call(**{name: None}) == 1, name
        for alias in (OUT, OUT2, H1):
            assert call(**{name: alias}) == 1, (name, hex(alias))
            assert b"must not alias" in lib.pf_last_error_string()
        assert call(**{name: OUT}, x0_prev=None, x0_out=None) == 1
    for alias in (X, EU, EC, OUT, OUT2):
        assert call(x0_out=alias) == 1, hex(alias)
    assert call(x0_prev=OUT) == 1 and call(x0_prev=OUT2) == 1
    assert call(out2=X) == 1 and call(out=EU) == 1
    assert call(rows=0) == 1 and call(W=0) == 1


# ------------------------------------------------------------------------------------------ DenoiseLoop: bad inputs
def test_loop_rejects_bad_known_inputs(fake_backend):
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion
    lat, pano, pe, ppe, cams = _inputs()
    k = _known(lat, pano, cams)
    mk = lambda **kw: KnownRegion(**dict(dict(latents=k.latents, mask=k.mask, pano_latent=k.pano_latent, pano_mask=k.pano_mask), **kw))
    loop = lambda known, lat=lat, pano=pano: DenoiseLoop(None, lat, pano, pe, ppe, cams, steps=4, known=known)
    bad = [mk(latents=k.latents[..., :8]), mk(mask=k.mask.expand(-1, -1, 4, -1, -1)), mk(mask=k.mask[:, :3]),
           mk(pano_latent=k.pano_latent[..., :16]), mk(pano_mask=k.pano_mask.expand(-1, -1, 4, -1, -1)),
           mk(pano_mask=k.pano_mask[..., :8, :]), mk(latents=None),
           mk(mask=k.mask * 1.5), mk(mask=k.mask - 0.1), mk(pano_mask=k.pano_mask + 0.01),
           mk(pano_mask=torch.where(k.pano_mask > 0, float("nan"), 0.0))]
    for i, known in enumerate(bad):
        with pytest.raises(ValueError):
            loop(known)
    # batch > 1: known content of two samples, or a loop over two samples
    two = lambda t: torch.cat([t, t])
    with pytest.raises(ValueError):
        loop(KnownRegion(two(k.latents), two(k.mask), two(k.pano_latent), two(k.pano_mask)))
    with pytest.raises(ValueError):
        loop(k, lat=two(lat), pano=two(pano))
    good = loop(k)
    assert good.mask_lat.shape == lat.shape and good.mask_pano.shape == pano.shape
    assert good.known_lat.dtype == good.noise_pano.dtype == good.mask_pano.dtype == torch.float32
    assert torch.equal(good.noise_lat, lat) and torch.equal(good.noise_pano, pano)     # the caller's frame, before the roll


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_known_loop_with_a_layout_condition(fake_backend, sampler):
    """A layout-conditioned loop (PanFusion.py:150-153) with known content: the condition image is still rolled with the panorama
    every step, the state is the same as without the condition for a denoiser that ignores it, and the kept entries end exact."""
    from panfusion_amd.pipeline import DenoiseLoop
    seen = []

    class Probe:
        def __call__(self, lat, pano, t, pe, ppe, cams, pers_cond=None, pano_cond=None):
            seen.append(None if pano_cond is None else pano_cond.clone())
            return 0.3 * lat + 0.1, 0.3 * pano - 0.2

    lat, pano, pe, ppe, cams = _inputs()
    known = _known(lat, pano, cams)
    cond = torch.rand(1, 1, 3, 128, 256, generator=torch.Generator().manual_seed(3))
    a = DenoiseLoop(Probe(), lat, pano, pe, ppe, cams, steps=5, sampler=sampler, known=known, pano_layout_cond=cond)
    b = DenoiseLoop(Probe(), lat, pano, pe, ppe, cams, steps=5, sampler=sampler, known=known)
    (lat_a, pano_a), (lat_b, pano_b) = a.run(), b.run()
    assert torch.equal(lat_a, lat_b) and torch.equal(pano_a, pano_b)
    for i, c in enumerate(seen[:5]):
        want = torch.roll(cond, int(90 / 360 * 256) * (i + 1), -1)
        assert torch.equal(c[0], want[0]) and torch.equal(c[1], want[0])
    keep = (known.pano_mask == 0).expand_as(pano_a)
    assert torch.equal(pano_a[keep], known.pano_latent[keep])
