"""fp32-source mode of the split-precision 1x1 GEMMs (pf_conv_desc.a_src_dtype = PF_F32; ops.conv_gemm_a32): the tile kernels read the
fp32 stream themselves and form the [hi | lo] pair of every K block in registers while they stage it, instead of reading a pair tensor
that a pass of its own (k_scale_shift_act) wrote.  The acceptance criterion is BIT IDENTITY with that two-launch form
(engine.split_operand + engine.exact_gemm): same affine map, same split, same plan, same MFMA order.  Needs an MI355X: `-m gpu`."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
D16 = [torch.float16, torch.bfloat16]
F32 = torch.float32


def ops():
    from panfusion_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


PLAN_FIELDS = ("kernel", "mrep", "nrep", "block_rows", "waves", "ring_slots", "splits", "kb_per_split", "m_split", "tail_splits", "tail_kb",
               "gn_rows", "n_tickets", "workspace_bytes")


def plan_tuple(g):
    return tuple(getattr(g, f) for f in PLAN_FIELDS)


def both_forms(dtype, x0, w, N, *, x1=None, scale=None, shift=None, n_img=1, bias=None, residual=None, out_dtype=F32, gn_stats=False):
    """(two-launch result, one-launch result, plan of the pair form, plan of the fp32-source form) of the same problem."""
    from panfusion_amd import engine
    o = ops()
    rows = x0.numel() // x0.shape[-1]
    w3 = engine._split_weight(w, 1, DEV, dtype)
    kw = dict(bias=bias, residual=residual, out_dtype=out_dtype, gn_stats=gn_stats)
    pair = engine.split_operand(x0, x1, scale, shift, 0, dtype=dtype)
    want = engine.exact_gemm(pair, w3, N, w_in=rows, **kw)
    g_pair = o.conv_gemm(pair, w3, N, c0=pair.shape[-1], a0_ld=pair.shape[-1], w_in=rows, split3=True, want_plan=True, **kw)
    got = o.conv_gemm_a32(x0, w3, N, dtype, x1=x1, scale=scale, shift=shift, n_img=n_img, **kw)
    g_a32 = o.conv_gemm_a32(x0, w3, N, dtype, x1=x1, scale=scale, shift=shift, n_img=n_img, want_plan=True, **kw)
    return want, got, g_pair, g_a32


def assert_identical(want, got):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want), "max |difference| %.3e" % float((got.float() - want.float()).abs().max())
    gw, gg = getattr(want, "_pf_gn", None), getattr(got, "_pf_gn", None)
    assert (gw is None) == (gg is None)
    if gw is not None:                                            # GroupNorm moments of the output, from the same epilogue
        assert gw[1] == gg[1] and torch.equal(gw[0], gg[0])


# ------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("dtype", D16)
def test_one_source_with_groupnorm_tile_spans_images(dtype):
    """3 images of 64 rows (the 8 x 8 level), C = 64, N = 160: a row tile holds rows of two images, each with its own scale / shift."""
    n, hw, Cc, N = 3, 64, 64, 160
    x = rnd(n, hw, Cc, seed=1, scale=2.0) + 0.5
    sc, sh = rnd(n, Cc, seed=2) * 0.3 + 1.0, rnd(n, Cc, seed=3)
    w, b = rnd(N, Cc, seed=4) / Cc ** 0.5, rnd(N, seed=5)
    want, got, gp, ga = both_forms(dtype, x, w, N, scale=sc, shift=sh, n_img=n, bias=b)
    assert_identical(want, got)
    assert plan_tuple(gp) == plan_tuple(ga)


@pytest.mark.parametrize("dtype", D16)
def test_two_sources_block_at_the_boundary_16bit_out(dtype):
    """x | skip with c0 = 96, c1 = 32: the K block of channels 64..95 ends source 0, the next one is all of source 1; 16-bit output."""
    rows, c0, c1, N = 200, 96, 32, 128
    x0, x1 = rnd(rows, c0, seed=6, scale=3.0), rnd(rows, c1, seed=7)
    w, b = rnd(N, c0 + c1, seed=8) / (c0 + c1) ** 0.5, rnd(N, seed=9)
    want, got, gp, ga = both_forms(dtype, x0, w, N, x1=x1, bias=b, out_dtype=dtype)
    assert want.dtype == dtype
    assert_identical(want, got)
    assert plan_tuple(gp) == plan_tuple(ga)


@pytest.mark.parametrize("dtype", D16)
def test_ragged_rows_128_wide_column_tile(dtype):
    """333 rows (no multiple of any row tile), N = 128: the 128-wide column tile; rows past M are staged as zeros and never stored."""
    rows, Cc, N = 333, 96, 128
    x = rnd(rows, Cc, seed=10)
    w = rnd(N, Cc, seed=11) / Cc ** 0.5
    guard = torch.full((rows + 64, N), 7.0, device=DEV)
    want, got, gp, ga = both_forms(dtype, x, w, N)
    assert_identical(want, got)
    from panfusion_amd import engine
    ops().conv_gemm_a32(x, engine._split_weight(w, 1, DEV, dtype), N, dtype, out=guard[:rows])
    assert torch.equal(guard[:rows], want) and bool((guard[rows:] == 7.0).all())
    assert plan_tuple(gp) == plan_tuple(ga) and gp.nrep == 4


@pytest.mark.parametrize("dtype", D16)
def test_small_m_long_k_split_k_residual_and_moments(dtype):
    """256 rows, C = 1280 (K = 2560), N = 320, fp32 output + fp32 residual + GroupNorm moments asked for: the split-K plan and its reduce.
    (Asked for, not emitted: a split-K plan and, by default, a launch with a residual have gn_rows = 0 in both forms, so the consumer's pass
    computes them -- the moments themselves are compared in test_groupnorm_moments_from_the_fp32_source_epilogue.)"""
    rows, Cc, N = 256, 1280, 320
    x = rnd(rows, Cc, seed=12)
    w, b, res = rnd(N, Cc, seed=13) / Cc ** 0.5, rnd(N, seed=14), rnd(rows, N, seed=15)
    want, got, gp, ga = both_forms(dtype, x, w, N, bias=b, residual=res, gn_stats=True)
    assert gp.splits > 1, plan_tuple(gp)
    assert_identical(want, got)
    assert plan_tuple(gp) == plan_tuple(ga)


# The split-precision 1x1 launches of the headline workload (proj_in and the resnet shortcuts of both branches; K = 2 C) by the kernel arm
# pf_conv_gemm_plan gives them, each with its N and K and the FEWEST rows that still select the arm (found with the plan query):
# (rows, N, K, (kernel, mrep, nrep, block_rows, waves, ring_slots, split K, tail split))
ARMS = [
    (32, 640, 640, (0, 2, 5, 64, 4, 2, False, False)),            # panorama 32 x 64: M4096 N640 K640 -- 4-wave kernel, unsplit
    (32, 640, 1280, (0, 2, 5, 64, 4, 2, True, False)),            # M4096 N640 K1280 / K1920, M1024 N1280 K1280, M256 N1280 K5120 -- 4-wave kernel, split K
    (3872, 1280, 1280, (1, 8, 5, 128, 4, 2, False, False)),       # M163840 N320 K640 / K1280, M40960 N640 K640 / K1280, M10240 N1280 K1280, M16384 N320 K640 / K1280
                                                                  # -- 8-wave kernel's 128-row blocks, two slots
    (8192, 640, 1920, (1, 8, 5, 256, 8, 3, False, False)),        # M163840 N320 K1920, M40960 N640 K1920 ... K3840, M16384 N320 K1920 -- 8 waves, three slots
    (8448, 1280, 2560, (1, 8, 5, 256, 8, 3, False, True)),        # M10240 N1280 K2560 ... K5120 -- whole rounds unsplit + a split-K tail launch
    (800, 1280, 2560, (1, 8, 5, 256, 8, 3, True, False)),         # M2560 N1280 K5120, M4096 N640 K2560 / K3840, M1024 N1280 K2560 ... K5120 -- 8 waves, split K
]


def arm_of(g):
    return (g.kernel, g.mrep, g.nrep, g.block_rows, g.waves, g.ring_slots, g.splits > 1, g.m_split > 0)


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("rows,N,K,arm", ARMS)
def test_every_arm_of_the_workload(rows, N, K, arm, dtype):
    Cc = K // 2
    x = rnd(rows, Cc, seed=16)
    w, b = rnd(N, Cc, seed=17) / Cc ** 0.5, rnd(N, seed=18)
    want, got, gp, ga = both_forms(dtype, x, w, N, bias=b)
    assert arm_of(ga) == arm, (arm_of(ga), arm)
    assert plan_tuple(gp) == plan_tuple(ga)
    assert_identical(want, got)


# proj_in's launches carry the GroupNorm scale / shift: on the 8-wave kernel that is an instantiation of its own (the scale / shift octet is requested
# behind the (W_lo, A_hi) group and joins the queue of the counted waits).  Every arm of it that exists, at the fewest rows that select the arm, with
# images whose boundaries fall inside a row tile: (images, rows per image, N, C, arm).  The 256 x 160 tile has no such instantiation (refused: the test below).
AFFINE_ARMS = [
    (2, 1936, 1280, 640, (1, 8, 5, 128, 4, 2, False, False)),     # proj_in of the workload at 64^2 / 32^2 and the panorama's 64 x 128: 128-row blocks, 160 columns
    (8, 2050, 256, 640, (1, 8, 4, 128, 4, 2, False, False)),      # 128-row blocks, 128 columns
    (8, 2050, 256, 960, (1, 8, 4, 256, 8, 3, False, False)),      # 256 x 128 tile, three slots, unsplit
    (5, 820, 256, 1280, (1, 8, 4, 256, 8, 3, True, False)),       # 256 x 128 tile, split K
]


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("n,hw,N,Cc,arm", AFFINE_ARMS)
def test_every_affine_arm_of_the_8_wave_kernel(n, hw, N, Cc, arm, dtype):
    x = rnd(n, hw, Cc, seed=19, scale=2.0) + 0.25
    sc, sh = rnd(n, Cc, seed=20) * 0.3 + 1.0, rnd(n, Cc, seed=21)
    w, b = rnd(N, Cc, seed=22) / Cc ** 0.5, rnd(N, seed=23)
    assert ops().conv_gemm_a32_serves(x, engine_split_weight(w, dtype), N, dtype, scale=sc, shift=sh, n_img=n)
    want, got, gp, ga = both_forms(dtype, x, w, N, scale=sc, shift=sh, n_img=n, bias=b)
    assert arm_of(ga) == arm, (arm_of(ga), arm)
    assert plan_tuple(gp) == plan_tuple(ga)
    assert_identical(want, got)


def engine_split_weight(w, dtype):
    from panfusion_amd import engine
    return engine._split_weight(w, 1, DEV, dtype)


def test_affine_map_on_the_256x160_tile_is_refused_and_reported():
    """The one arm without an affine instantiation (no registers for the scale / shift octet): the plan query says so, the launch is refused
    before anything runs, and engine.exact_gemm_f32 takes the two-launch form there."""
    from panfusion_amd import engine
    from panfusion_amd._lib import PanFusionHipError
    o = ops()
    n, hw, N, Cc = 2, 4096, 640, 960                             # (8192, 640, 1920): 8 waves, 256 x 160, three slots
    x = rnd(n, hw, Cc, seed=24)
    sc, sh = rnd(n, Cc, seed=25) * 0.3 + 1.0, rnd(n, Cc, seed=26)
    w = rnd(N, Cc, seed=27) / Cc ** 0.5
    w3 = engine_split_weight(w, torch.float16)
    assert not o.conv_gemm_a32_serves(x, w3, N, torch.float16, scale=sc, shift=sh, n_img=n)
    out = torch.full((n * hw, N), 5.0, device=DEV)
    with pytest.raises(PanFusionHipError):
        o.conv_gemm_a32(x, w3, N, torch.float16, scale=sc, shift=sh, n_img=n, out=out)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    got = engine.exact_gemm_f32(x, w3, N, torch.float16, scale=sc, shift=sh, w_in=n * hw, out_dtype=F32)
    want = engine.exact_gemm(engine.split_operand(x, None, sc, sh, 0, dtype=torch.float16), w3, N, w_in=n * hw, out_dtype=F32)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", D16)
@pytest.mark.parametrize("affine", [False, True])
def test_groupnorm_moments_from_the_fp32_source_epilogue(dtype, affine):
    """A plan that DOES emit the moments of its output (4-wave kernel, unsplit, no residual; images are whole 32-row runs), with a ragged last
    row tile (288 rows in 64-row tiles): rows past M are staged as zeros -- as `shift` under the affine map -- and must not reach the sums.
    (The split-K case above cannot carry moments: a split plan has gn_rows = 0, as has every launch with a residual by default.)"""
    n, hw, Cc, N = 3, 96, 64, 160
    x = rnd(n, hw, Cc, seed=28, scale=2.0)
    sc, sh = (rnd(n, Cc, seed=29) * 0.3 + 1.0, rnd(n, Cc, seed=30) + 3.0) if affine else (None, None)
    w, b = rnd(N, Cc, seed=31) / Cc ** 0.5, rnd(N, seed=32)
    want, got, gp, ga = both_forms(dtype, x, w, N, scale=sc, shift=sh, n_img=n if affine else 1, bias=b, gn_stats=True)
    assert ga.kernel == 0 and ga.splits == 1 and ga.gn_rows == 32 and gp.gn_rows == 32, (plan_tuple(gp), plan_tuple(ga))
    assert getattr(want, "_pf_gn", None) is not None and getattr(got, "_pf_gn", None) is not None
    assert_identical(want, got)
    # the moments are those of the stored output: per 32-row run and column pair
    ref = got.double().view(-1, 32, N // 2, 2)
    # (bound: a sum of 64 fp32 terms in any order is within 63 u sum|v| of the exact one, u = 2^-24)
    err = (got._pf_gn[0][:, 0].double() - ref.sum((1, 3))).abs()
    assert bool((err <= 63 * 2.0 ** -24 * ref.abs().sum((1, 3)) + 1e-30).all()), float(err.max())


# ------------------------------------------------------------------------------------ 2. accuracy against float64
@pytest.mark.parametrize("dtype", D16)
def test_fp32_source_gemm_reproduces_fp32(dtype):
    """The inputs and the gates of test_gpu_mixed.test_split_precision_gemm_reproduces_fp32 (1x1 over a channel concat of two streams)."""
    from panfusion_amd import engine
    n, hw, c0, c1, N = 4, 32 * 32, 640, 320, 320
    x0, x1 = rnd(n, hw, c0, seed=30, scale=2.0), rnd(n, hw, c1, seed=31)
    w = rnd(N, c0 + c1, seed=32) / (c0 + c1) ** 0.5
    b = rnd(N, seed=33)
    want = torch.cat([x0, x1], -1).reshape(-1, c0 + c1).double() @ w.double().T + b.double()
    got = ops().conv_gemm_a32(x0, engine._split_weight(w, 1, DEV, dtype), N, dtype, x1=x1, bias=b, out_dtype=F32)
    e = rel_l2(got.cpu(), want.float().cpu())
    print("fp32-source split-precision 1x1 %s: %.2e" % (dtype, e))
    assert e <= (2e-6 if dtype == torch.float16 else 4e-5)


# ------------------------------------------------------------------------------------ 3. module level
@pytest.fixture(scope="module")
def small_unet():
    """A mixed-precision UNet at the benchmark's --small widths (64, 128, 256, 256), packed once."""
    from oracle import sd2_unet as U
    from panfusion_amd import engine
    cfg = U.tiny_config(width=64, cross_attention_dim=128, heads=(1, 2, 4, 4), groups=32)
    unet = U.UNet2DConditionModel(**cfg)
    U.init_synthetic(unet, 7)
    return engine.pack_unet(unet, DEV, torch.float16, mixed=True)


def _on_and_off(monkeypatch, run):
    """run() with the one-launch form and with PF_A32=0's two-launch form; -> (results, one-launch GEMMs issued)."""
    from panfusion_amd import engine
    o = ops()
    calls, real = [], o.conv_gemm_a32

    def counted(*a, **kw):
        if not kw.get("want_plan"):                               # (a plan query launches nothing)
            calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(o, "conv_gemm_a32", counted)
    monkeypatch.setattr(engine, "A32", True)
    on = run()
    n_on = len(calls)
    monkeypatch.setattr(engine, "A32", False)
    off = run()
    assert len(calls) == n_on, "PF_A32=0 still took the one-launch form"
    return on, off, n_on


@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_run_transformer_is_bit_identical_with_and_without(small_unet, monkeypatch, h, w):
    from panfusion_amd import engine
    u = small_unet
    text = rnd(2, 7, 128, seed=40).half()
    for i, t in enumerate([u.down[0].attns[0], u.down[1].attns[1], u.mid.attns[0], u.up[3].attns[2]]):
        Cc = t.norm.g.shape[0]
        x = rnd(2, h, w, Cc, seed=41 + i, scale=1.5)
        on, off, n_on = _on_and_off(monkeypatch, lambda: engine.run_transformer(t, x, text))
        assert n_on == 1 and on.dtype == F32 and torch.isfinite(on).all()
        assert torch.equal(on, off), "C = %d" % Cc


@pytest.mark.parametrize("h,w", [(8, 8), (16, 16)])
def test_run_resnet_is_bit_identical_with_and_without(small_unet, monkeypatch, h, w):
    """Resnets with a 1x1 shortcut: a down-block one (one source), decoder ones (x | skip), and a panorama one through the virtual
    circular padding (wrap = 2: the shortcut reads the un-padded x | skip)."""
    from panfusion_amd import engine
    u = small_unet
    n = 2
    temb = rnd(n, u.temb_total, seed=50)
    cases = [(u.down[1].resnets[0], 0, 0), (u.up[0].resnets[0], 256, 0), (u.up[2].resnets[2], 64, 0), (u.up[3].resnets[0], 128, 2),
             (u.up[1].resnets[2], 128, 2)]
    for i, (r, c_skip, wrap) in enumerate(cases):
        assert r.ws3 is not None and r.cin > c_skip
        x = rnd(n, h, w, r.cin - c_skip, seed=51 + i, scale=1.5)
        skip = rnd(n, h, w, c_skip, seed=61 + i) if c_skip else None
        on, off, n_on = _on_and_off(monkeypatch, lambda: engine.run_resnet(r, x, skip, temb, wrap=wrap))
        assert n_on == 1 and on.dtype == F32 and on.shape == (n, h, w, r.cout) and torch.isfinite(on).all()
        assert torch.equal(on, off), "cin %d cout %d wrap %d" % (r.cin, r.cout, wrap)


# ------------------------------------------------------------------------------------ 4. graph replay
def test_transformer_graph_replays_equal_eager_under_contention(small_unet):
    """One transformer block (its proj_in on the one-launch form) captured into a graph: three replays, each beside an unrelated GEMM on a
    second stream, equal the eager result bit for bit (the form of test_linear_ws_is_bit_reproducible_under_contention; run once)."""
    from panfusion_amd import engine
    assert engine.A32
    t = small_unet.down[1].attns[0]
    x = rnd(2, 16, 16, t.norm.g.shape[0], seed=70, scale=1.5)
    text = rnd(2, 7, 128, seed=71).half()
    eager = engine.run_transformer(t, x, text).clone()          # (also the warm-up: plans, kernel attributes)
    torch.cuda.synchronize()
    side, big = torch.cuda.Stream(), torch.randn(4096, 4096, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = engine.run_transformer(t, x, text)
    for it in range(3):
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            big @ big
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager), "replay %d differs from the eager run" % it


# ------------------------------------------------------------------------------------ 5. argument rejection
def test_bad_arguments_are_rejected_before_any_launch():
    from panfusion_amd import engine
    from panfusion_amd._lib import PanFusionHipError
    o = ops()
    rows, Cc, N = 128, 64, 128
    x, sc = rnd(rows, Cc + 4, seed=80), rnd(1, Cc, seed=81)
    w3 = engine._split_weight(rnd(N, Cc, seed=82), 1, DEV, torch.float16)
    w9 = engine._split_weight(rnd(N, 9 * Cc, seed=83), 9, DEV, torch.float16)
    out = torch.full((rows, N), 5.0, device=DEV)

    def rejected(call):
        with pytest.raises(PanFusionHipError):
            call()
        torch.cuda.synchronize()
        assert bool((out == 5.0).all()), "something was launched"

    xc = x[:, :Cc].contiguous()
    # ksize = 3 with an fp32 source
    rejected(lambda: o.conv_gemm(xc.view(1, 8, 16, Cc), w9, N, n_img=1, h_in=8, w_in=16, ksize=3, pad=1, split3=True, a32_dtype=torch.float16,
                                 out=out))
    # c0 % 32 != 0
    rejected(lambda: o.conv_gemm(xc, w3, N, c0=48, c1=None, split3=True, a32_dtype=torch.float16, out=out))
    # a scale without a shift
    rejected(lambda: o.conv_gemm(xc, w3, N, split3=True, a32_dtype=torch.float16, a_scale=sc, out=out))
    # a misaligned source (4 bytes past a 16-byte boundary; leading dimension Cc + 4)
    rejected(lambda: o.conv_gemm(x[:, 1:Cc + 1], w3, N, c0=Cc, a0_ld=Cc + 4, split3=True, a32_dtype=torch.float16, out=out))
    # (and the form that is accepted, with the same buffers)
    o.conv_gemm(xc, w3, N, split3=True, a32_dtype=torch.float16, out=out)
    assert torch.isfinite(out).all() and not bool((out == 5.0).all())
