"""Two-pass high-resolution sampling, host side: SourceLatents(..., resample=).check()'s accept / reject matrix,
the loop on the test double tests/fake_ops.py with a low-resolution source against the same loop fed a full-size source that
torch up-sampled in the naive tripled form, the launch count of loops whose sources have the loop's size, HiResLoop against the
hand composition of two loops, the sharded loop over gloo, and the C entry point's argument checks (no launch, no GPU)."""
import ctypes as C
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import fake_ops
from conftest import build_tiny_oracle, rel_l2
from test_inpaint_cpu import _inputs
from test_strength_cpu import START_OP, _noise, _same, _source
from test_strength_cpu import _use_fake_backend as _strength_backend

HERE = os.path.dirname(os.path.abspath(__file__))
UP_OP = {"enabled": False, "calls": []}


def tripled(z, size, mode):
    """Periodic columns, stated naively: three copies side by side, torch's resize, the middle one."""
    kw = {} if mode == "nearest" else dict(align_corners=False)
    W = size[1]
    flat = z.reshape(-1, 1, *z.shape[-2:])
    r = F.interpolate(torch.cat([flat] * 3, -1), size=(size[0], 3 * W), mode=mode, **kw)[..., W:2 * W]
    return r.reshape(tuple(z.shape[:-2]) + tuple(size))


def clamped(z, size, mode):
    kw = {} if mode == "nearest" else dict(align_corners=False)
    r = F.interpolate(z.reshape(-1, 1, *z.shape[-2:]), size=tuple(size), mode=mode, **kw)
    return r.reshape(tuple(z.shape[:-2]) + tuple(size))


def upsampled_start_pair(z, noise, ka, kb, roll=0, *, mode, wrap, out, out2=None, tstep=None, t0=0):
    """Torch stand-in for ops.upsampled_start_pair, set on the fake_ops module at run time.  It raises unless a test enabled it:
    a loop whose sources have the loop's size must never get here."""
    if not UP_OP["enabled"]:
        raise AssertionError("upsampled_start_pair called by a loop that must not use it")
    UP_OP["calls"].append(dict(src=tuple(z.shape), mode=mode, wrap=wrap, roll=roll, noise=noise is not None))
    r = (tripled if wrap else clamped)(z, out.shape[-2:], mode)
    y = torch.roll(r if noise is None else ka * r + kb * noise, roll, -1)
    out.copy_(y)
    if out2 is not None:
        out2.copy_(y)
    if tstep is not None:
        tstep.fill_(int(t0))
    return out


def _use_fake_backend(put, extra=()):
    _strength_backend(put, extra)
    put(fake_ops, "upsampled_start_pair", upsampled_start_pair)


@pytest.fixture
def fake_backend(monkeypatch):
    _use_fake_backend(lambda o, n, v: monkeypatch.setattr(o, n, v, raising=False), ["panfusion_amd.sharding"])
    monkeypatch.setitem(START_OP, "enabled", True)                # noised_start_pair: every strength < 1 loop uses it
    monkeypatch.setitem(START_OP, "calls", [])
    monkeypatch.setitem(UP_OP, "enabled", False)
    monkeypatch.setitem(UP_OP, "calls", [])
    return monkeypatch


@pytest.fixture
def up_op(fake_backend):
    fake_backend.setitem(UP_OP, "enabled", True)
    return UP_OP["calls"]


@pytest.fixture(scope="module")
def oracle_model():
    return build_tiny_oracle()


def _low(lat, pano, cams, fv=(2, 2), fp=(2, 2), seed=5, resample="bicubic"):
    """A seeded source smaller than (lat, pano) by the factors fv (views) and fp (panorama)."""
    from oracle import ddim as oddim
    from panfusion_amd.pipeline import SourceLatents
    H, W = pano.shape[-2:]
    h, w = lat.shape[-2:]
    z = torch.randn(1, 1, 4, H // fp[0], W // fp[1], generator=torch.Generator().manual_seed(seed))
    return SourceLatents(oddim.init_noise(z, cams, h // fv[0], w // fv[1])[1], z, resample=resample)


def _full(low, lat, pano):
    """The full-size source of the naive restatement: torch's resize, the panorama in the tripled form."""
    from panfusion_amd.pipeline import SourceLatents
    return SourceLatents(clamped(low.latents, lat.shape[-2:], low.resample), tripled(low.pano_latent, pano.shape[-2:], low.resample))


# ------------------------------------------------------------------------------------------------------- check()
def test_source_check_accepts_integer_factors_only():
    from panfusion_amd.pipeline import SourceLatents
    lat, pano = torch.empty(1, 4, 4, 16, 16, device="meta"), torch.empty(1, 1, 4, 16, 32, device="meta")
    z = lambda *s: torch.zeros(*s)
    ok = [((1, 4, 4, 16, 16), (1, 1, 4, 16, 32)), ((1, 4, 4, 8, 8), (1, 1, 4, 8, 16)), ((1, 4, 4, 16, 16), (1, 1, 4, 8, 16)),
          ((1, 4, 4, 4, 8), (1, 1, 4, 16, 8)), ((1, 4, 4, 1, 1), (1, 1, 4, 2, 32)), ((1, 4, 4, 8, 16), (1, 1, 4, 16, 32))]
    for mode in ("nearest", "bilinear", "bicubic"):
        for sv, sp in ok:
            SourceLatents(z(*sv), z(*sp), resample=mode).check(lat, pano)
    bad = [((1, 4, 4, 6, 16), (1, 1, 4, 16, 32)),              # 16 / 6 is not an integer
           ((1, 4, 4, 16, 16), (1, 1, 4, 16, 12)),             # 32 / 12
           ((1, 4, 4, 32, 32), (1, 1, 4, 16, 32)),             # larger than the loop
           ((1, 3, 4, 8, 8), (1, 1, 4, 8, 16)),                # another m
           ((1, 4, 3, 8, 8), (1, 1, 4, 8, 16)),                # another channel count
           ((1, 4, 4, 8, 8), (1, 1, 3, 8, 16)),
           ((2, 4, 4, 8, 8), (2, 1, 4, 8, 16)),                # batch
           ((4, 4, 8, 8), (1, 1, 4, 8, 16))]                   # rank
    for sv, sp in bad:
        with pytest.raises(ValueError):
            SourceLatents(z(*sv), z(*sp), resample="bicubic").check(lat, pano)
    with pytest.raises(ValueError):
        SourceLatents(None, z(1, 1, 4, 8, 16), resample="bilinear").check(lat, pano)
    with pytest.raises(ValueError):                               # resample=None: today's rule, any mismatch raises
        SourceLatents(z(1, 4, 4, 8, 8), z(1, 1, 4, 8, 16)).check(lat, pano)
    with pytest.raises(ValueError):
        SourceLatents(z(1, 4, 4, 16, 16), z(1, 1, 4, 8, 16)).check(lat, pano)
    SourceLatents(z(1, 4, 4, 16, 16), z(1, 1, 4, 16, 32)).check(lat, pano)
    for mode in ("lanczos", "area", "", 2, True):
        with pytest.raises(ValueError):
            SourceLatents(z(1, 4, 4, 8, 8), z(1, 1, 4, 8, 16), resample=mode)
    with pytest.raises(ValueError):                               # batch 2 loop
        SourceLatents(z(2, 4, 4, 8, 8), z(2, 1, 4, 8, 16), resample="bicubic").check(torch.empty(2, 4, 4, 16, 16, device="meta"),
                                                                                     torch.empty(2, 1, 4, 16, 32, device="meta"))


# ------------------------------------------------------------------------------------------ the loop on the fake backend
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("rot_diff", [90.0, 37.0])
@pytest.mark.parametrize("mode", ["bicubic", "bilinear", "nearest"])
def test_lowres_source_loop_matches_naive_restatement(up_op, oracle_model, sampler, rot_diff, mode):
    """n = 10 at strength 0.6: the loop fed a half-size source equals, at the start and after every step, the loop fed the
    full-size source torch made of it (views plain, panorama in the tripled form), within 1e-4 rel-L2 -- the bound
    test_strength_cpu.test_strength_loop_matches_naive_restatement uses -- and that full-size loop equals test_strength_cpu's
    restatement of diffusers' img2img loop within the same bound."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    from test_strength_cpu import restated
    lat, pano, pe, ppe, cams = _inputs()
    low = _low(lat, pano, cams, resample=mode)
    full = _full(low, lat, pano)
    make = lambda init: DenoiseLoop(hip_model(oracle_model), lat, pano, pe, ppe, cams, steps=10, rot_diff=rot_diff,
                                    sampler=sampler, strength=0.6, init=init)
    a = make(low)
    assert [(c["wrap"], c["mode"], c["noise"]) for c in up_op] == [(False, mode, True), (True, mode, True)]
    assert [c["roll"] for c in up_op] == [0, a.shift] and a.src_pano.shape == low.pano_latent.shape
    del up_op[:]
    b = make(full)
    assert up_op == []
    start, want = restated(oracle_model, lat, pano, pe, ppe, cams, full.latents, full.pano_latent, None, 10, 0.6, sampler, rot_diff)
    es = [rel_l2(a.lat, b.lat), rel_l2(a.pano, b.pano), rel_l2(a.lat, start[0]), rel_l2(torch.roll(a.pano, -a.shift, -1), start[1])]
    assert max(es) < 1e-4, es
    assert torch.equal(a.lat2[0], a.lat2[1]) and torch.equal(a.pano2[0], a.pano2[1]) and torch.equal(a.tstep, b.tstep)
    for j in range(6):
        a.step()
        b.step()
        moved = 0 if j == 5 else a.shift
        es = [rel_l2(a.lat, b.lat), rel_l2(a.pano, b.pano), rel_l2(a.lat, want[j][0]),
              rel_l2(torch.roll(a.pano, -moved, -1), want[j][1])]
        assert max(es) < 1e-4, (sampler, rot_diff, mode, j + 1, es)
    # the wrap is really in effect: a clamped panorama source starts elsewhere at the seam
    seam = rel_l2(tripled(low.pano_latent, pano.shape[-2:], mode)[..., :2], clamped(low.pano_latent, pano.shape[-2:], mode)[..., :2])
    assert mode == "nearest" or seam > 1e-2


def test_full_size_sources_never_call_the_new_op(fake_backend, oracle_model):
    """The stand-in of the new op is NOT enabled here and raises if called: loops built with defaults, with a full-size source
    (with or without resample=), at strength 1 with a low-resolution source, and their restarts."""
    from panfusion_amd.pipeline import DenoiseLoop, SourceLatents
    lat, pano, pe, ppe, cams = _inputs()
    src = _source(lat, pano, cams)
    make = lambda **kw: DenoiseLoop(_zero_model, lat, pano, pe, ppe, cams, steps=5, **kw)
    make().run()
    for init in (src, SourceLatents(src.latents, src.pano_latent, resample="bicubic")):
        loop = make(strength=0.6, init=init)
        loop.run()
        loop.restart(init=init, strength=0.4)
        loop.run()
    low = _low(lat, pano, cams)
    loop = make(strength=1.0, init=low)                            # the start is the noise: the source is only stored
    assert torch.equal(loop.lat, lat) and loop.src_pano.shape == low.pano_latent.shape
    loop.run()
    assert UP_OP["calls"] == [] and len(START_OP["calls"]) == 8
    with pytest.raises(AssertionError):                            # and the stand-in does guard
        loop.restart(strength=0.6)
    with pytest.raises(AssertionError):
        make(strength=0.6, init=low)


def _zero_model(lat2, pano2, *a):
    return torch.zeros_like(lat2), torch.zeros_like(pano2)


def test_restart_takes_a_source_of_another_size(up_op, oracle_model):
    """restart(init=) with a source of another admissible size equals a fresh loop bit for bit; a refused one changes nothing."""
    from panfusion_amd.pipeline import DenoiseLoop, SourceLatents
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    model = hip_model(oracle_model)
    make = lambda init, s=0.6: DenoiseLoop(model, lat, pano, pe, ppe, cams, steps=5, strength=s, init=init)
    src = _source(lat, pano, cams)
    loop = make(src)
    ptrs = [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep)]
    loop.run()
    low = _low(lat, pano, cams, fv=(1, 1), fp=(2, 4), seed=8, resample="bilinear")
    loop.restart(init=low)
    assert loop.src_pano.shape == (1, 1, 4, 8, 8) and loop.src_lat.shape == lat.shape and loop.resample == "bilinear"
    assert [c["wrap"] for c in up_op] == [True]                    # the views have the loop's size: the existing launch
    assert _same(loop.run(), make(low).run())
    with pytest.raises(ValueError):
        loop.restart(init=SourceLatents(low.latents, low.pano_latent[..., :5], resample="bilinear"))
    with pytest.raises(ValueError):
        loop.restart(init=SourceLatents(low.latents, low.pano_latent))
    assert loop.src_pano.shape == (1, 1, 4, 8, 8) and loop.resample == "bilinear"
    loop.restart(init=src, strength=0.8)                           # and back to a full-size one
    assert loop.resample is None and _same(loop.run(), make(src, 0.8).run())
    assert ptrs == [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep)]


# ------------------------------------------------------------------------------------------------------ HiResLoop
def _hires_inputs(same_views):
    """(base noise pair, final noise pair): the tiny loop's inputs as the FINAL size, a base of half the size -- or, with
    same_views, a base panorama of half the size under views of the final size (the 512x1024 -> 1024x2048 shape of things)."""
    from oracle import ddim as oddim
    lat, pano, pe, ppe, cams = _inputs()
    H, W = pano.shape[-2:]
    h, w = lat.shape[-2:]
    n_p = torch.randn(1, 1, 4, H // 2, W // 2, generator=torch.Generator().manual_seed(31))
    hv, wv = (h, w) if same_views else (h // 2, w // 2)
    return (oddim.init_noise(n_p, cams, hv, wv)[1], n_p), (lat, pano)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("same_views", [False, True])
def test_hires_loop_equals_two_loops_by_hand(up_op, oracle_model, sampler, same_views):
    from panfusion_amd.pipeline import DenoiseLoop, HiResLoop, SourceLatents
    from test_engine_logic_cpu import hip_model
    lat, pano, pe, ppe, cams = _inputs()
    model = hip_model(oracle_model)
    base_noise, noise = _hires_inputs(same_views)
    kw = dict(steps=4, refine_steps=6, strength=0.5, resample="bicubic", sampler=sampler)

    def by_hand(base_noise, noise, strength=0.5):
        base = DenoiseLoop(model, *base_noise, pe, ppe, cams, steps=4, sampler=sampler)
        z = base.run()
        return DenoiseLoop(model, *noise, pe, ppe, cams, steps=6, sampler=sampler, strength=strength,
                           init=SourceLatents(*z, resample="bicubic")).run()
    want = [t.clone() for t in by_hand(base_noise, noise)]
    del up_op[:]
    loop = HiResLoop(model, base_noise, noise, pe, ppe, cams, **kw)
    assert loop.base.steps == 4 and len(loop.base.timesteps) == 4 and len(loop.refine.timesteps) == 3
    got = [t.clone() for t in loop.run()]
    assert _same(got, want) and _same(loop.result(), want)
    assert got[0].shape == lat.shape and got[1].shape == pano.shape
    if same_views:                                                 # the views' source is passed through without resampling
        assert up_op and all(c["wrap"] for c in up_op) and loop.refine.src_lat.shape == lat.shape
    else:
        assert [c["wrap"] for c in up_op[-2:]] == [False, True]
    ptrs = [t.data_ptr() for lp in (loop.base, loop.refine) for t in (lp.lat2, lp.pano2, lp.tstep)]
    loop.restart()
    assert loop.base.i == 0 and loop.refine.i == 0
    assert _same(loop.run(), want)
    loop.restart(base_noise, noise)
    assert _same(loop.run(), want)
    new_base = _noise(*base_noise, cams, 41)
    loop.restart(base_noise=new_base)
    other = [t.clone() for t in loop.run()]
    assert not _same(other, want) and _same(other, by_hand(new_base, noise))
    new = _noise(lat, pano, cams, 42)
    loop.restart(noise=new, strength=0.7)
    assert len(loop.refine.timesteps) == 4
    assert _same(loop.run(), by_hand(new_base, new, 0.7))
    assert ptrs == [t.data_ptr() for lp in (loop.base, loop.refine) for t in (lp.lat2, lp.pano2, lp.tstep)]


def test_hires_loop_rejects_bad_inputs(up_op):
    from panfusion_amd.pipeline import HiResLoop
    lat, pano, pe, ppe, cams = _inputs()
    base_noise, noise = _hires_inputs(False)
    make = lambda b=base_noise, n=noise, **kw: HiResLoop(_zero_model, b, n, pe, ppe, cams, **dict(dict(steps=4), **kw))
    for kw in (dict(strength=1.0), dict(strength=0.0), dict(strength=0.1), dict(resample="lanczos"), dict(resample=None),
               dict(b=(base_noise[0][..., :6], base_noise[1])), dict(b=noise, n=base_noise), dict(sampler="euler")):
        with pytest.raises(ValueError):
            make(**kw)
    loop = make()
    for kw in (dict(strength=1.0), dict(strength=0.1), dict(noise=base_noise), dict(base_noise=noise),
               dict(base_noise=(base_noise[0], None), noise=(noise[0][..., :4], None))):
        with pytest.raises(ValueError):
            loop.restart(**kw)
    assert loop.refine.strength == 0.5
    loop.run()


# --------------------------------------------------------------------------------------- sharded loop over gloo
def _sharded_scenario(make):
    """A half-size source at strength 0.6, 2M; one step, then a restart with a bilinear source of other factors, run."""
    lat, pano, pe, ppe, cams = args = _inputs()
    loop = make(args, steps=5, sampler="dpmpp_2m", strength=0.6, init=_low(lat, pano, cams))
    first = [t.clone() for t in loop.run()]
    loop.restart(init=_low(lat, pano, cams, fv=(2, 1), fp=(1, 4), seed=9, resample="bilinear"), strength=0.8)
    return first, [t.clone() for t in loop.run()]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    _use_fake_backend(setattr, ["panfusion_amd.sharding"])
    START_OP["enabled"] = UP_OP["enabled"] = True
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from panfusion_amd import sharding
        from test_engine_logic_cpu import hip_model
        model = hip_model(build_tiny_oracle())
        make = lambda args, **kw: sharding.ShardedDenoiseLoop(model, sharding.make_shard(4), *args, **kw)
        torch.save(_sharded_scenario(make), os.path.join(out, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_sharded_loop_with_a_lowres_source_equals_single_process(up_op):
    """World 2: every rank holds the full latents and sources, so the sharded loop with a low-resolution source equals the
    single-process loop on every rank (1e-4 rel-L2, the bound of test_strength_cpu's sharded test) and the replicas are
    bit-identical."""
    from panfusion_amd.pipeline import DenoiseLoop
    from test_engine_logic_cpu import hip_model
    from test_sharding_gloo import _free_port
    world = 2
    model = hip_model(build_tiny_oracle())
    single = _sharded_scenario(lambda args, **kw: DenoiseLoop(model, *args, **kw))
    with tempfile.TemporaryDirectory() as out:
        mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    for r in res:
        for got, want in zip(r, single):
            assert rel_l2(got[0], want[0]) < 1e-4 and rel_l2(got[1], want[1]) < 1e-4
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])
    assert not _same(single[0], single[1])


# ------------------------------------------------------------------------------------- C entry point: argument checks
def test_entry_point_rejects_bad_arguments_before_launching():
    """Validation happens before any launch (fake, never dereferenced device addresses; every call below must fail)."""
    from panfusion_amd import _lib
    lib = _lib.lib()
    Z, N, OUT, OUT2, T = (0x10000 * i for i in range(1, 6))

    def call(z=Z, noise=N, planes=4, h=32, w=64, H=64, W=128, mode=2, wrap=1, out=OUT, out2=OUT2, tstep=None, n_tstep=0):
        return lib.pf_upsampled_start_pair(z, noise, C.c_float(0.6), C.c_float(0.8), planes, h, w, H, W, mode, wrap, 3, out, out2,
                                           tstep, n_tstep, 501, None)
    err = lib.pf_last_error_string
    assert call(out=None) == 1 and b"pf_upsampled_start_pair" in err()
    assert call(z=None) == 1 and b"pf_upsampled_start_pair" in err()
    assert call(W=96) == 1 and b"pf_upsampled_start_pair" in err() and b"integer" in err()       # 96 / 64
    assert call(H=48) == 1 and b"integer" in err()
    assert call(h=64, H=32) == 1 and b"integer" in err()                                         # smaller than the source
    assert call(w=1024, W=4096) == 1 and b"pf_upsampled_start_pair" in err() and b"2048" in err()
    assert call(w=2049, W=2049) == 1 and b"2048" in err()
    assert call(mode=3) == 1 and b"mode" in err() and call(mode=-1) == 1
    assert call(out2=OUT) == 1 and b"out2" in err()
    assert call(out=Z) == 1 and b"alias" in err()
    assert call(out2=Z) == 1 and call(out=N) == 1 and call(out2=N) == 1
    assert call(tstep=T, n_tstep=0) == 1 and b"n_tstep" in err()
    assert call(planes=0) == 1 and call(h=0) == 1 and call(w=0) == 1 and call(H=0) == 1 and call(W=0) == 1
    assert call(planes=1 << 31) == 1
