"""Strength < 1 sampling from a source panorama and DenoiseLoop.restart() on the MI355X: pf_noised_start_pair
against a float64 torch statement, the rolled copy and the blend kernel's operand bit for bit; the two cfg 1 trajectories against
the fixtures tools/make_golden_strength.py wrote with the reference class as the denoiser (diffusers' form: add_noise start,
sliced timesteps, everything rolled with the state); restart() under graph replay; one short cfg 2 run from an encoded panorama.
Needs an MI355X: `-m gpu`."""
import pytest
import torch

from conftest import cam4, golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("shape", [(1, 20, 4, 64, 64), (1, 1, 4, 64, 128), (1, 1, 4, 128, 256)])
def test_noised_start_pair_vs_float64(shape):
    """cfg 2's view and panorama latents and a 256-wide panorama; rolls 0, W/4, 17, -5: out within 2e-6 rel-L2 of
    roll(ka z + kb n) in float64 (fp32 coefficients) -- the bound test_inpaint_step_pair_vs_float64 uses for the same arithmetic
    -- out2 == out bit for bit, the timestep words written; z = NULL is roll_width(noise) bit for bit; and with the (ka, kb) of a
    step the result is what pf_cfg_inpaint_step_pair writes at mask = 0 with the same pair, bit for bit (the shared fmaf)."""
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DDIMSchedule
    sched = DDIMSchedule()
    grid = sched.set_timesteps(10)
    W = shape[-1]
    z, n = rnd(*shape, seed=61), rnd(*shape, seed=62)
    x, eu, ec = (rnd(*shape, seed=63 + j).to(DEV) for j in range(3))
    zd, nd = z.to(DEV), n.to(DEV)
    f32 = lambda c: float(torch.tensor(c, dtype=torch.float32))
    for t, roll in zip(grid[1::2], (0, W // 4, 17, -5)):
        coef = sched.coefficients(t)
        ka, kb = coef[:2]
        want = torch.roll(f32(ka) * z.double() + f32(kb) * n.double(), roll, -1)
        pair = torch.full((2,) + shape[1:], float("nan"), device=DEV)
        tstep = torch.full((2, 5), 7, dtype=torch.long, device=DEV)
        out = ops.noised_start_pair(zd, nd, ka, kb, roll, out=pair[:1], out2=pair[1:], tstep=tstep, t0=t)
        assert out.data_ptr() == pair.data_ptr()
        e = rel_l2(out.cpu(), want)
        print("noised_start_pair %s roll %d: rel-L2 vs float64 %.2e" % (shape, roll, e))
        assert e <= 2e-6, (shape, roll, e)
        assert torch.equal(pair[0], pair[1])
        assert torch.equal(tstep.cpu(), torch.full((2, 5), t, dtype=torch.long))
        # without out2 / tstep
        single = ops.noised_start_pair(zd, nd, ka, kb, roll, out=torch.empty_like(zd))
        assert torch.equal(single, pair[:1])
        # z = NULL: the rolled noise, bit for bit
        tstep.fill_(7)
        copy = ops.noised_start_pair(None, nd, 0.0, 0.0, roll, out=pair[:1], out2=pair[1:])
        assert torch.equal(copy, ops.roll_width(nd, roll)) and torch.equal(pair[0], pair[1])
        assert torch.equal(tstep.cpu(), torch.full((2, 5), 7, dtype=torch.long))
        # the blend kernel's operand r = fmaf(ka, z, kb n): mask = 0 writes it
        blend, _ = ops.cfg_inpaint_step_pair(x, eu, ec, 9.0, coef, roll, known=zd, noise=nd, mask=torch.zeros_like(zd), ka=ka,
                                             kb=kb, known_roll=0)
        assert torch.equal(blend, single)


def test_noised_start_pair_rejects_bad_arguments():
    from panfusion_amd import _lib, ops
    z, n, out, out2 = (torch.zeros(1, 4, 8, 64, device=DEV) for _ in range(4))
    with pytest.raises(_lib.PanFusionHipError, match="16384"):
        wide = torch.zeros(1, 16385, device=DEV)
        ops.noised_start_pair(wide, wide.clone(), 0.6, 0.8, out=wide.clone())
    for kw in (dict(out=z), dict(out=n), dict(out=out, out2=out), dict(out=out, out2=n)):
        with pytest.raises(_lib.PanFusionHipError):
            ops.noised_start_pair(z, n, 0.6, 0.8, 3, **kw)
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


FIXTURES = {"ddim": "cfg1_strength06_ddim10.npz", "dpmpp_2m": "cfg1_strength06_inpaint_dpmpp10.npz"}


def _fixture_loop(model, gd, sampler, graphs, noise=None, strength=0.6):
    """The cfg 1 loop of a fixture: DDIM from SourceLatents without a mask, or 2M with the kept band (the source is the known
    latents: init=None)."""
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion, SourceLatents
    t = lambda k: torch.from_numpy(gd[k]).to(DEV)
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    if noise is not None:
        latents, pano_latent = noise
    known = init = None
    if "known_mask" in gd:
        known = KnownRegion(t("source_latents"), t("known_mask"), t("source_pano"), t("known_pano_mask"))
    else:
        init = SourceLatents(t("source_latents"), t("source_pano"))
    return DenoiseLoop(model, latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=10, use_graphs=graphs,
                       sampler=sampler, known=known, init=init, strength=strength)


def _trajectory(loop):
    """(views, panorama in the un-rotated frame) after every executed step, as DenoiseLoop.result un-rolls it."""
    from panfusion_amd import ops
    traj = []
    for _ in range(len(loop.timesteps)):
        loop.step()
        traj.append((loop.lat.clone(), ops.roll_width(loop.pano, int(-loop.total_rot / 360 * loop.W)).clone()))
    return traj


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_cfg1_strength06_vs_oracle(full_width, sampler, graphs):
    """BASELINE.json configs[0] (m = 4 views of 32x32 latents + the 64x128 panorama latent, SD-2-base widths, guidance 9, 90 degrees
    per step) on the 10-step grid at strength 0.6 -- 6 steps from t = 501 -- against the fixtures of tools/make_golden_strength.py
    (the reference class as the denoiser): DDIM without a mask, and 2M with the seam-crossing kept band (first order at the first
    executed step and at the last).  Start state and the state after EVERY step, views and panorama, within 1e-3 rel-L2: the
    north_star gate the DDIM, 2M and inpaint trajectories are held to.  Kept entries equal the known latents bit for bit after
    result().  Drift per step is printed with -s."""
    from panfusion_amd import ops
    gd = golden(FIXTURES[sampler])
    loop = _fixture_loop(_hip_model(full_width), gd, sampler, graphs)
    assert loop.timesteps == [int(t) for t in gd["timesteps"]] == [501, 401, 301, 201, 101, 1]
    w = lambda k, i=None: torch.from_numpy(gd[k] if i is None else gd[k][i])
    start = (rel_l2(loop.lat.cpu(), w("start_latents")), rel_l2(ops.roll_width(loop.pano, -loop.shift).cpu(), w("start_pano")))
    assert torch.equal(loop.lat2[0], loop.lat2[1]) and torch.equal(loop.pano2[0], loop.pano2[1])
    assert torch.equal(loop.tstep.cpu(), torch.full((2, 4), 501, dtype=torch.long))
    traj = _trajectory(loop)
    drift = [(rel_l2(v.cpu(), w("latents", i)), rel_l2(p.cpu(), w("pano_latent", i))) for i, (v, p) in enumerate(traj)]
    print("\ncfg1 strength 0.6 %s drift, graphs %s (views / pano rel-L2; start, then per step):" % (sampler, graphs))
    print("  start: %.2e/%.2e  " % start + "  ".join("%d: %.2e/%.2e" % (i + 1, a, b) for i, (a, b) in enumerate(drift)))
    lat, pano = loop.result()
    assert torch.equal(lat, traj[-1][0]) and torch.equal(pano, traj[-1][1])
    if loop.known is not None:
        known = loop.known
        keep_v = (known.mask == 0).expand_as(lat)
        keep_p = (known.pano_mask == 0).expand_as(pano)
        assert int(keep_v.sum()) > 0 and int(keep_p.sum()) == 4 * 64 * 56
        assert torch.equal(lat[keep_v], known.latents[keep_v]) and torch.equal(pano[keep_p], known.pano_latent[keep_p])
    assert start[0] <= 1.0e-3 and start[1] <= 1.0e-3, start
    for i, (a, b) in enumerate(drift):
        assert a <= 1.0e-3 and b <= 1.0e-3, (sampler, graphs, i + 1, a, b)


def test_restart_replays_the_same_graphs(full_width):
    """2M with known content at strength 0.6, graphs on: after a full run, restart() + run reproduces a fresh loop bit for bit --
    with the same inputs and with new noise and a new strength -- and the graph entries are the very same objects (no capture)."""
    from oracle import ddim as oddim
    from oracle import fixtures as FX
    gd = golden(FIXTURES["dpmpp_2m"])
    model = _hip_model(full_width)
    loop = _fixture_loop(model, gd, "dpmpp_2m", True)
    first = [t.clone() for t in loop.run()]
    fresh = _fixture_loop(model, gd, "dpmpp_2m", True).run()
    assert all(torch.equal(a, b) for a, b in zip(first, fresh))
    graphs = dict(loop.graphs)
    ptrs = [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep, loop.x0_lat, loop.x0_pano)]
    assert len(graphs) == 4
    loop.restart()
    assert all(torch.equal(a, b) for a, b in zip(loop.run(), first))
    n_p = rnd(1, 1, 4, 64, 128, seed=71)
    noise = (oddim.init_noise(n_p, FX.horizon4_cameras(), 32, 32)[1], n_p)
    loop.restart(noise[0].to(DEV), noise[1].to(DEV), strength=0.8)
    got = [t.clone() for t in loop.run()]
    want = _fixture_loop(model, gd, "dpmpp_2m", True, noise=noise, strength=0.8).run()
    assert len(loop.timesteps) == 8 and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not all(torch.equal(a, b) for a, b in zip(got, first))
    assert sorted(loop.graphs) == sorted(graphs) and all(loop.graphs[k] is graphs[k] for k in graphs)
    assert ptrs == [t.data_ptr() for t in (loop.lat2, loop.pano2, loop.tstep, loop.x0_lat, loop.x0_pano)]


def test_restart_of_a_plain_loop_with_graphs(full_width):
    """"Next seed, same prompt": a text-to-panorama loop built with defaults, restarted with new noise, equals a fresh loop."""
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop
    model = _hip_model(full_width)
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    make = lambda la, pa: DenoiseLoop(model, la.to(DEV), pa.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=4, use_graphs=True)
    loop = make(rnd(*latents.shape, seed=72), rnd(*pano_latent.shape, seed=73))
    loop.run()
    graphs = dict(loop.graphs)
    loop.restart(latents.to(DEV), pano_latent.to(DEV))
    got = loop.run()
    assert all(torch.equal(a, b) for a, b in zip(got, make(latents, pano_latent).run()))
    assert all(loop.graphs[k] is graphs[k] for k in graphs) and len(loop.graphs) == len(graphs)


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


def test_source_from_panorama_encodes_as_known_region_does(tiny_encoder):
    from panfusion_amd.pipeline import KnownRegion, SourceLatents
    pano = (torch.rand(1, 1, 3, 128, 256, generator=torch.Generator().manual_seed(12)) * 2 - 1).to(DEV)
    cams = {k: v[None] for k, v in cam4().items()}
    src = SourceLatents.from_panorama(tiny_encoder, pano, cams, (8, 8))
    k = KnownRegion.from_panorama(tiny_encoder, pano, torch.ones(1, 1, 1, 128, 256, device=DEV), cams, (8, 8))
    assert src.latents.shape == (1, 4, 4, 8, 8) and src.pano_latent.shape == (1, 1, 4, 16, 32)
    assert torch.equal(src.latents, k.latents) and torch.equal(src.pano_latent, k.pano_latent)
    with pytest.raises(ValueError):
        SourceLatents.from_panorama(tiny_encoder, pano[0], cams, (8, 8))


def test_cfg2_strength_half_from_an_encoded_panorama(full_width, tiny_encoder):
    """cfg 2 geometry (20 icosahedron views of 64x64 latents + the 64x128 panorama latent, SD-2-base widths, graphs), a 6-step grid
    at strength 0.5 from SourceLatents.from_panorama of a synthetic 512x1024 panorama: 3 steps run, everything finite."""
    from oracle import fixtures as FX
    from panfusion_amd.pipeline import DenoiseLoop, SourceLatents
    n = 6
    cams = FX.ico_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (64, 64), (64, 128))
    pano = (torch.rand(1, 1, 3, 512, 1024, generator=torch.Generator().manual_seed(15)) * 2 - 1).to(DEV)
    src = SourceLatents.from_panorama(tiny_encoder, pano, cams, (64, 64))
    loop = DenoiseLoop(_hip_model(full_width), latents.to(DEV), pano_latent.to(DEV), pe.to(DEV), ppe.to(DEV), cams, steps=n,
                       use_graphs=True, strength=0.5, init=src)
    assert len(loop.timesteps) == int(n / 2) and loop.timesteps == loop.sched.set_timesteps(n)[n // 2:]
    loop.prepare()
    lat, pano_out = loop.run()
    assert loop.i == 3 and torch.isfinite(lat).all() and torch.isfinite(pano_out).all()
    assert lat.shape == latents.shape and pano_out.shape == pano_latent.shape
