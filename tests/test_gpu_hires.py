"""Two-pass high-resolution sampling on the MI355X: pf_upsampled_start_pair against a float64 torch statement
(the panorama in the naive tripled form), its bit-for-bit properties (the unfused pair it replaces, factor 1, roll equivariance,
where wrap and clamp differ), the cfg 1 refine trajectory against the fixture tools/make_golden_hires.py wrote with the reference
class as the denoiser, and HiResLoop at SD-2-base widths under graph replay.  Needs an MI355X: `-m gpu`."""
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("nearest", "bilinear", "bicubic")
RADIUS = {"nearest": 0, "bilinear": 1, "bicubic": 2}              # source columns a tap may lie beyond the edge


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def torch_resize(z, size, mode, wrap):
    """torch's own resize of (..., h, w) in z's dtype on the CPU; wrap: three copies side by side, resized, the middle one."""
    kw = {} if mode == "nearest" else dict(align_corners=False)
    flat = z.reshape(-1, 1, *z.shape[-2:])
    W = size[1]
    if wrap:
        r = F.interpolate(torch.cat([flat] * 3, -1), size=(size[0], 3 * W), mode=mode, **kw)[..., W:2 * W]
    else:
        r = F.interpolate(flat, size=tuple(size), mode=mode, **kw)
    return r.reshape(tuple(z.shape[:-2]) + tuple(size))


CASES = [((1, 1, 4, 64, 128), (128, 256), True), ((1, 20, 4, 32, 32), (64, 64), False), ((1, 1, 4, 32, 64), (96, 256), True)]


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,size,wrap", CASES)
def test_upsampled_start_pair_vs_float64(src, size, wrap, mode):
    """The 2x panorama, the 2x views and a 3 x 4 panorama; rolls 0, W/4, 17, -5: out within 2e-6 rel-L2 of
    roll(ka r + kb n) in float64 (fp32 coefficients), r = F.interpolate in float64 on the CPU in the tripled (wrapped) or plain
    (clamped) form -- the bound test_noised_start_pair_vs_float64 holds the same fmaf to -- out2 == out bit for bit, the timestep
    words written; the pure resize (noise = None) within the same bound of r."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DDIMSchedule
    sched = DDIMSchedule()
    grid = sched.set_timesteps(10)
    shape = src[:3] + size
    W = size[1]
    z, n = rnd(*src, seed=91), rnd(*shape, seed=92)
    zd, nd = z.to(DEV), n.to(DEV)
    r64 = torch_resize(z.double(), size, mode, wrap)
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))
    for t, roll in zip(grid[1::2], (0, W // 4, 17, -5)):
        ka, kb = sched.coefficients(t)[:2]
        want = torch.roll(f32(ka) * r64 + f32(kb) * n.double(), roll, -1)
        pair = torch.full((2,) + shape[1:], float("nan"), device=DEV)
        tstep = torch.full((2, 5), 7, dtype=torch.long, device=DEV)
        out = ops.upsampled_start_pair(zd, nd, ka, kb, roll, mode=mode, wrap=wrap, out=pair[:1], out2=pair[1:], tstep=tstep, t0=t)
        assert out.data_ptr() == pair.data_ptr()
        e = rel_l2(out.cpu(), want)
        print("upsampled_start_pair %s -> %s %s wrap %s roll %d: rel-L2 vs float64 %.2e" % (src, size, mode, wrap, roll, e))
        assert e <= 2e-6, (src, size, mode, roll, e)
        assert torch.equal(pair[0], pair[1])
        assert torch.equal(tstep.cpu(), torch.full((2, 5), t, dtype=torch.long))
        single = ops.upsampled_start_pair(zd, nd, ka, kb, roll, mode=mode, wrap=wrap, out=torch.empty_like(nd))
        assert torch.equal(single, pair[:1])
    r = ops.resize_latent(zd, size, mode, wrap)
    e = rel_l2(r.cpu(), r64)
    e32 = rel_l2(torch_resize(z, size, mode, wrap), r64)
    print("resize_latent %s -> %s %s wrap %s: rel-L2 vs float64 %.2e (torch's fp32 path: %.2e)" % (src, size, mode, wrap, e, e32))
    assert r.shape == shape and e <= 2e-6, (src, size, mode, e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,size,wrap", CASES)
def test_fused_launch_equals_resize_then_noised_start_bit_for_bit(src, size, wrap, mode):
    """upsampled_start_pair(z, n, ka, kb, roll) == noised_start_pair(resize_latent(z), n, ka, kb, roll): r is complete before
    the shared fmaf."""
    from panfusion_amd import ops
    shape = src[:3] + size
    zd, nd = rnd(*src, seed=93).to(DEV), rnd(*shape, seed=94).to(DEV)
    for roll in (0, size[1] // 4, 17, -5):
        fused = ops.upsampled_start_pair(zd, nd, 0.6123, 0.7906, roll, mode=mode, wrap=wrap, out=torch.empty_like(nd))
        pair = ops.noised_start_pair(ops.resize_latent(zd, size, mode, wrap), nd, 0.6123, 0.7906, roll, out=torch.empty_like(nd))
        assert torch.equal(fused, pair), (mode, roll)


@pytest.mark.parametrize("mode", MODES)
def test_factor_one_returns_the_source_bit_for_bit(mode):
    from panfusion_amd import ops
    for shape, wrap in (((1, 1, 4, 64, 128), True), ((1, 20, 4, 32, 32), False), ((1, 1, 4, 64, 128), False)):
        zd = rnd(*shape, seed=95).to(DEV)
        assert torch.equal(ops.resize_latent(zd, shape[-2:], mode, wrap), zd)
        assert torch.equal(ops.upsampled_start_pair(zd, None, 0.0, 0.0, 9, mode=mode, wrap=wrap, out=torch.empty_like(zd)),
                           ops.roll_width(zd, 9))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,size", [((1, 1, 4, 64, 128), (128, 256)), ((1, 1, 4, 32, 64), (96, 256)), ((1, 1, 4, 16, 24), (16, 1992))])
def test_rolling_the_source_rolls_the_wrapped_output(src, size, mode):
    """Phase weights: resize(roll(z, k)) == roll(resize(z), k fw) bit for bit with wrap=True, for every k tried -- also at fw = 83
    and W = 1992, where a running fp32 source coordinate has long lost its last bits."""
    from panfusion_amd import ops
    zd = rnd(*src, seed=96).to(DEV)
    fw = size[1] // src[-1]
    ref = ops.resize_latent(zd, size, mode, True)
    for k in (1, 5, src[-1] // 2, src[-1] - 1, -3):
        got = ops.resize_latent(torch.roll(zd, k, -1).contiguous(), size, mode, True)
        assert torch.equal(got, torch.roll(ref, k * fw, -1)), (mode, k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,size", [((1, 1, 4, 64, 128), (128, 256)), ((1, 1, 4, 32, 64), (96, 256))])
def test_wrap_and_clamp_differ_only_at_the_edge_columns(src, size, mode):
    """Outside the columns whose taps reach beyond the source's first or last column the two forms are the same arithmetic; inside
    they differ on random data (not for nearest, which has no tap beyond its own sample)."""
    from panfusion_amd import ops
    zd = rnd(*src, seed=97).to(DEV)
    fw, W = size[1] // src[-1], size[1]
    a, b = ops.resize_latent(zd, size, mode, True), ops.resize_latent(zd, size, mode, False)
    edge = RADIUS[mode] * fw
    assert torch.equal(a[..., edge:W - edge], b[..., edge:W - edge])
    if edge:
        assert not torch.equal(a[..., :edge], b[..., :edge]) and not torch.equal(a[..., W - edge:], b[..., W - edge:])
        assert float((a[..., 0] - b[..., 0]).abs().max()) > 1e-2 and float((a[..., -1] - b[..., -1]).abs().max()) > 1e-2
    else:
        assert torch.equal(a, b)


def test_upsampled_start_pair_rejects_bad_arguments():
    from panfusion_amd import _lib, ops
    z = torch.zeros(1, 4, 8, 64, device=DEV)
    out, out2, n = (torch.zeros(1, 4, 16, 128, device=DEV) for _ in range(3))
    with pytest.raises(_lib.PanFusionHipError, match="2048"):
        ops.resize_latent(torch.zeros(1, 1, 2, 1025, device=DEV), (2, 2050))
    with pytest.raises(_lib.PanFusionHipError, match="integer"):
        ops.resize_latent(z, (16, 96))
    with pytest.raises(ValueError):
        ops.resize_latent(z, (16, 128), mode="area")
    for kw in (dict(out=out, out2=out), dict(out=n), dict(out=out, out2=n)):
        with pytest.raises(_lib.PanFusionHipError):
            ops.upsampled_start_pair(z, n, 0.6, 0.8, 3, mode="bicubic", wrap=True, **kw)
    wide = ops.resize_latent(torch.ones(1, 1, 2, 512, device=DEV), (4, 2048), wrap=True)          # the limit itself runs
    torch.cuda.synchronize()
    assert wide.shape == (1, 1, 4, 2048) and float((wide - 1).abs().max()) < 1e-6


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


@pytest.mark.parametrize("graphs", [False, True])
def test_cfg1_hires_refine_vs_oracle(full_width, graphs):
    """BASELINE.json configs[0] (m = 4 views of 32x32 latents + the 64x128 panorama latent, SD-2-base widths, guidance 9, 90 degrees
    per step) on the 10-step grid at strength 0.6 -- 6 DDIM steps from t = 501 -- from the HALF-SIZE source of
    tools/make_golden_hires.py through SourceLatents(..., resample="bicubic"): the views take the clamped form, the panorama the
    wrapped one.  Start state and the state after EVERY step, views and panorama, within 1e-3 rel-L2 of the fixture (torch's
    bicubic, the panorama tripled, then the reference class as the denoiser): the north_star gate of the other trajectories.
    Drift per step is printed with -s."""
    from oracle import fixtures as FX
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DenoiseLoop, SourceLatents
    gd = golden("cfg1_hires_ddim10.npz")
    w = lambda k, i=None: torch.from_numpy(gd[k] if i is None else gd[k][i])
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    init = SourceLatents(w("lowres_latents").to(DEV), w("lowres_pano").to(DEV), resample="bicubic")
    assert init.latents.shape == (1, 4, 4, 16, 16) and init.pano_latent.shape == (1, 1, 4, 32, 64)
    loop = DenoiseLoop(_hip_model(full_width), latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=10,
                       use_graphs=graphs, init=init, strength=0.6)
    assert loop.timesteps == [int(t) for t in gd["timesteps"]] == [501, 401, 301, 201, 101, 1]
    src = (rel_l2(ops.resize_latent(init.latents, (32, 32), "bicubic", False).cpu(), w("source_latents")),
           rel_l2(ops.resize_latent(init.pano_latent, (64, 128), "bicubic", True).cpu(), w("source_pano")))
    start = (rel_l2(loop.lat.cpu(), w("start_latents")), rel_l2(ops.roll_width(loop.pano, -loop.shift).cpu(), w("start_pano")))
    assert torch.equal(loop.lat2[0], loop.lat2[1]) and torch.equal(loop.pano2[0], loop.pano2[1])
    assert torch.equal(loop.tstep.cpu(), torch.full((2, 4), 501, dtype=torch.long))
    drift = []
    for i in range(6):
        loop.step()
        pano = ops.roll_width(loop.pano, int(-loop.total_rot / 360 * loop.W))
        drift.append((rel_l2(loop.lat.cpu(), w("latents", i)), rel_l2(pano.cpu(), w("pano_latent", i))))
    print("\ncfg1 hires refine drift, graphs %s (views / pano rel-L2; up-sampled source, start, then per step):" % graphs)
    print("  source: %.2e/%.2e  start: %.2e/%.2e  " % (src + start)
          + "  ".join("%d: %.2e/%.2e" % (i + 1, a, b) for i, (a, b) in enumerate(drift)))
    lat, pano = loop.result()
    assert rel_l2(lat.cpu(), w("latents", 5)) == drift[-1][0] and rel_l2(pano.cpu(), w("pano_latent", 5)) == drift[-1][1]
    assert max(src) <= 1.0e-3 and start[0] <= 1.0e-3 and start[1] <= 1.0e-3, (src, start)
    for i, (a, b) in enumerate(drift):
        assert a <= 1.0e-3 and b <= 1.0e-3, (graphs, i + 1, a, b)


def test_hires_loop_full_width_with_graphs(full_width):
    """cfg 1 -> a 128x256 panorama latent under the same four 32x32 views, 3 + 3 steps, graphs on: finite; equal to the hand
    composition of two loops bit for bit; restart() + run() reproduces it bit for bit with both loops' graph entries the very
    same objects; new noise changes it."""
    from oracle import ddim as oddim
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop, HiResLoop, SourceLatents
    model = _hip_model(full_width)
    cams = FX.horizon4_cameras()
    b_lat, b_pano, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    n_pano = rnd(1, 1, 4, 128, 256, seed=98)
    n_lat = oddim.init_noise(n_pano, cams, 32, 32)[1]
    dev = lambda *ts: tuple(t.to(DEV) for t in ts)
    pe, ppe = dev(pe, ppe)
    loop = HiResLoop(model, dev(b_lat, b_pano), dev(n_lat, n_pano), pe, ppe, cams, steps=3, refine_steps=6, strength=0.5,
                     use_graphs=True)
    loop.prepare()
    assert len(loop.base.graphs) == 4 and len(loop.refine.graphs) == 4 and len(loop.refine.timesteps) == 3
    assert loop.refine.src_lat.shape == b_lat.shape and loop.refine.src_pano.shape == b_pano.shape
    graphs = [dict(loop.base.graphs), dict(loop.refine.graphs)]
    first = [t.clone() for t in loop.run()]
    assert first[0].shape == n_lat.shape and first[1].shape == n_pano.shape
    assert all(torch.isfinite(t).all() for t in first)
    # by hand
    base = DenoiseLoop(model, *dev(b_lat, b_pano), pe, ppe, cams, steps=3, use_graphs=True)
    z = base.run()
    hand = DenoiseLoop(model, *dev(n_lat, n_pano), pe, ppe, cams, steps=6, use_graphs=True, strength=0.5,
                       init=SourceLatents(*z, resample="bicubic")).run()
    assert all(torch.equal(a, b) for a, b in zip(first, hand))
    ptrs = lambda: [t.data_ptr() for lp in (loop.base, loop.refine) for t in (lp.lat2, lp.pano2, lp.tstep, lp.src_lat, lp.src_pano)
                    if t is not None]
    before = ptrs()
    loop.restart()
    assert all(torch.equal(a, b) for a, b in zip(loop.run(), first))
    loop.restart(dev(b_lat, b_pano), dev(n_lat, n_pano))
    assert all(torch.equal(a, b) for a, b in zip(loop.run(), first))
    n_pano2 = rnd(1, 1, 4, 128, 256, seed=99)
    loop.restart(noise=dev(oddim.init_noise(n_pano2, cams, 32, 32)[1], n_pano2))
    other = loop.run()
    assert all(torch.isfinite(t).all() for t in other) and not any(torch.equal(a, b) for a, b in zip(other, first))
    for lp, g in zip((loop.base, loop.refine), graphs):
        assert sorted(lp.graphs) == sorted(g) and all(lp.graphs[k] is g[k] for k in g)
    assert ptrs() == before
