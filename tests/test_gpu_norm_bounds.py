"""The normalisation kernels of pf_elementwise.hip against float64, per ELEMENT and per (image, group): the three producers of
GroupNorm statistics (direct, two-stage, from a GEMM epilogue's column-pair moments), the apply kernel in every (input type,
output kind) its host dispatch accepts, and LayerNorm(+PE) in both row forms.  Bounds, caps, inputs and case tables are
tests/norm_model.py's (derived there from the kernels' loops; tests/test_norm_bounds_cpu.py holds the CPU side).  Needs an
MI355X: `-m gpu`.

Everything goes through panfusion_amd.ops and reaches its arm through the shape alone.  Sources are views at a non-zero,
16-byte aligned storage offset of buffers whose surroundings hold a canary that would wreck the statistics; outputs that take
out= are the middle of NaN-filled buffers whose guard regions must stay NaN."""
import pytest
import torch

import norm_model as M
from conftest import unpair

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                 # canary / guard elements on either side (128 or 256 bytes: the views stay 16-byte aligned)
CANARY = 3.0e4           # finite in all three types; one of them read as a pixel moves a group's moments by orders of magnitude


def ops():
    from panfusion_amd import ops as o
    return o


def dev_view(t, fill=CANARY):
    """CPU tensor -> contiguous device view of the same shape inside a larger buffer filled with `fill`."""
    if t is None:
        return None
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t.to(DEV))
    assert v.data_ptr() % 16 == 0 and v.storage_offset() > 0
    return v


def nan_out(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def guards_intact(buf, name):
    torch.cuda.synchronize()
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all(), "%s: wrote outside its output" % name


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def ratio(got, want, bound):
    return M.worst((got.detach().double().cpu() - want).abs(), bound)


# ------------------------------------------------------------------------------------------------ GroupNorm statistics + apply
@pytest.mark.parametrize("dtype", M.ALL3, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("i", range(len(M.GN_CASES)), ids=[c.name for c in M.GN_CASES])
def test_groupnorm_statistics_and_apply(i, dtype):
    c, x, ref = M.gn_ref(i, dtype)
    name = "%s %s" % (c.name, M.DT_ID[dtype])
    x0, x1 = dev_view(x.x0), dev_view(x.x1)
    sc, sh = ops().groupnorm_scale_shift(x0, x1, c.n, c.hw, c.groups, 1e-5, x.gamma.to(DEV), x.beta.to(DEV), wrap=c.wrap)
    out_dtype = torch.float16 if dtype == torch.float32 else dtype
    buf, out = nan_out((c.n, c.hw, c.c0 + c.c1), out_dtype)
    y = ops().scale_shift_act(x0, x1, c.n, c.hw, sc, sh, 1, out=out, out_dtype=out_dtype)
    guards_intact(buf, name)
    sc, sh, y = sc.cpu(), sh.cpu(), y.cpu()
    dS, dH = M.gn_stat_bounds(ref, c.L, x.gamma, x.beta)
    want, bound = M.gn_end_to_end_bound(x.x, ref, sc, sh, dS, dH, 1, out_dtype)
    print("RATIO %-9s %-46s %-4s L %3d  scale |err| / bound %.3f  shift %.3f  (|d scale| / |scale| - 2u) / (kappa u) %.3f of cap %.2f  y %.3f"
          % (c.arm, c.name, M.DT_ID[dtype], c.L, ratio(sc, ref.scale, dS), ratio(sh, ref.shift, dH), float(M.excess_ratio(sc, ref).max()),
             M.CAP[c.arm], ratio(y, want, bound)))
    M.assert_within(name + " scale", sc, ref.scale, dS)
    M.assert_within(name + " shift", sh, ref.shift, dH)
    M.assert_cap(name, sc, ref, c.arm)
    M.assert_within(name + " GroupNorm + SiLU", y, want, bound)


# ------------------------------------------------------------------------------------------------ statistics from column-pair moments
@pytest.mark.parametrize("i", range(len(M.PART_CASES)), ids=[c.name for c in M.PART_CASES])
def test_groupnorm_from_partials(i):
    c = M.PART_CASES[i]
    x = M.part_inputs(c, seed=i)
    C = c.c0 + c.c1
    x0, x1 = dev_view(x.x0), dev_view(x.x1)
    gam, bet = x.gamma.to(DEV), x.beta.to(DEV)
    if not c.usable:
        # moments that must not be used (an odd number of channel pairs per group / runs that straddle the images): all NaN
        x0._pf_gn = (torch.full((c.n * cdiv(c.hw, c.rows0), 2, c.c0 // 2), float("nan"), device=DEV), c.rows0)
        sc, sh = ops().groupnorm_scale_shift(x0, None, c.n, c.hw, c.groups, 1e-5, gam, bet)
        sc, sh = sc.cpu(), sh.cpu()
        ref = M.gn_reference(x.x, c.groups, x.gamma, x.beta)
        arm, L = M.gn_chain(c.n, c.hw, C, c.groups)
        dS, dH = M.gn_stat_bounds(ref, L, x.gamma, x.beta)
        print("RATIO partials  %-46s fp32 refused -> %s: scale |err| / bound %.3f  shift %.3f  excess %.3f of cap %.2f"
              % (c.name, arm, ratio(sc, ref.scale, dS), ratio(sh, ref.shift, dH), float(M.excess_ratio(sc, ref).max()), M.CAP[arm]))
        M.assert_within(c.name + " scale", sc, ref.scale, dS)
        M.assert_within(c.name + " shift", sh, ref.shift, dH)
        M.assert_cap(c.name, sc, ref, arm)
        return
    parts = [M.make_partials(x.x0, c.rows0)] + ([M.make_partials(x.x1, c.rows1)] if c.c1 else [])
    cs = [c.c0] + ([c.c1] if c.c1 else [])
    # the sources themselves must not be read: poisoned
    x0.fill_(float("nan"))
    x0._pf_gn = (dev_view(parts[0], float("nan")), c.rows0)
    if c.c1:
        x1.fill_(float("nan"))
        x1._pf_gn = (dev_view(parts[1], float("nan")), c.rows1)
    sc, sh = ops().groupnorm_scale_shift(x0, x1, c.n, c.hw, c.groups, 1e-5, gam, bet)
    sc, sh = sc.cpu(), sh.cpu()
    ref = M.partials_reference(parts, cs, c.n, c.hw, c.groups, x.gamma, x.beta)
    dS, dH = M.partials_bounds(ref, max(c.hw // c.rows0, c.hw // c.rows1), x.beta)
    print("RATIO partials  %-46s fp32 gpb %d pairs %3d slices %3d  scale |err| / (u |scale|) %.3f of 2  shift |err| / bound %.3f"
          % (c.name, c.gpb, c.npairs, c.slices, float(((sc.double() - ref.scale).abs() / (M.U32 * ref.scale.abs())).max()), ratio(sh, ref.shift, dH)))
    M.assert_within(c.name + " scale", sc, ref.scale, dS)
    M.assert_within(c.name + " shift", sh, ref.shift, dH)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ apply
def apply_inputs(shape, tin, seed):
    n, hw, c0, c1 = shape
    g = torch.Generator().manual_seed(6000 + seed)
    x = torch.randn(n, hw, c0 + c1, generator=g) * 2 + 0.5
    x[:, hw - 1, c0 + c1 - 1] += M.OUTLIER                          # the clamped duplicate octet of the last thread reads this one
    x[:, 0, c0 % (c0 + c1)] -= M.OUTLIER
    x = x.to(tin)
    sc = torch.randn(n, c0 + c1, generator=g) * 0.5 + 1
    sh = torch.randn(n, c0 + c1, generator=g)
    return x, sc, sh


def check_pair(name, pair, v32, t16):
    """hi == round16(v32), lo == round16(v32 - hi), bit for bit."""
    hi, lo = unpair(pair.cpu())
    want_hi = v32.to(t16)
    want_lo = (v32 - want_hi.float()).to(t16)
    bad_hi, bad_lo = int((bits(hi) != bits(want_hi)).sum()), int((bits(lo) != bits(want_lo)).sum())
    assert bad_hi == 0 and bad_lo == 0, "%s: %d hi and %d lo of %d differ from round16(y32), round16(y32 - hi)" % (name, bad_hi, bad_lo, hi.numel())


@pytest.mark.parametrize("act", [1, 0], ids=["silu", "affine"])
@pytest.mark.parametrize("combo", M.APPLY_COMBOS, ids=["%s-%s-%s" % (M.DT_ID[a], M.DT_ID[b], k) for a, b, k in M.APPLY_COMBOS])
def test_apply(combo, act):
    tin, tout, kind = combo
    shape = M.APPLY_SHAPES[kind]
    n, hw, c0, c1 = shape
    C = c0 + c1
    assert kind != "plain" or (hw * (C // 8)) % 2 == 1               # odd per_img: the last thread's second octet is the clamped duplicate
    name = "apply %s->%s %s act%d" % (M.DT_ID[tin], M.DT_ID[tout], kind, act)
    x, sc, sh = apply_inputs(shape, tin, M.APPLY_COMBOS.index(combo))
    x0, x1 = dev_view(x[..., :c0].contiguous()), dev_view(x[..., c0:].contiguous())
    scd, shd = dev_view(sc, float("nan")), dev_view(sh, float("nan"))
    buf, out = nan_out((n, hw, C * (2 if kind == "split" else 1)), tout)
    got = ops().scale_shift_act(x0, x1, n, hw, scd, shd, act, out=out, out_dtype=tout, split=kind == "split", raw_pair=kind == "raw")
    guards_intact(buf, name)
    want32, bound32 = M.apply_bound(x, sc, sh, act, torch.float32)
    if kind == "plain":
        want, bound = M.apply_bound(x, sc, sh, act, tout)
        r = M.assert_within(name, got.cpu(), want, bound)
    else:
        # the fp32 output of the same inputs: inside the fp32 bound, and the 16-bit results are its roundings bit for bit
        b32, o32 = nan_out((n, hw, C), torch.float32)
        y32 = ops().scale_shift_act(x0, x1, n, hw, scd, shd, act, out=o32, out_dtype=torch.float32)
        guards_intact(b32, name + " (fp32)")
        y32 = y32.cpu()
        r = M.assert_within(name + " (fp32 output)", y32, want32, bound32)
        if kind == "split":
            check_pair(name, got, y32, tout)
        else:
            y, pair = got
            assert bool((bits(y.cpu()) == bits(y32.to(tout))).all()), name + ": y != round16(y32)"
            check_pair(name + " raw pair", pair, x.float(), tout)
    print("RATIO apply     %-46s worst |err| / bound %.3f" % (name, r))


@pytest.mark.parametrize("tin", M.ALL3, ids=["bf16", "fp16", "fp32"])
def test_apply_without_scale_single_source(tin):
    n, hw, C = 2, 77, 104
    tout = torch.float16 if tin == torch.float32 else tin
    x, _, _ = apply_inputs((n, hw, C, 0), tin, 50)
    x0 = dev_view(x)
    for act in (1, 0):
        buf, out = nan_out((n, hw, C), tout)
        y = ops().scale_shift_act(x0, None, n, hw, None, None, act, out=out, out_dtype=tout)
        guards_intact(buf, "apply without scale")
        want, bound = M.apply_bound(x, None, None, act, tout)
        r = M.assert_within("apply without scale %s act%d" % (M.DT_ID[tin], act), y.cpu(), want, bound)
        print("RATIO apply     %-46s worst |err| / bound %.3f" % ("scale=None %s->%s act%d" % (M.DT_ID[tin], M.DT_ID[tout], act), r))
        if not act and tin == tout:
            assert bool((bits(y.cpu()) == bits(x)).all()), "identity must copy bit for bit"


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("types", M.LN_TYPES, ids=["%s-%s" % (M.DT_ID[a], M.DT_ID[b]) for a, b in M.LN_TYPES])
@pytest.mark.parametrize("i", range(len(M.LN_CASES)), ids=[c.name for c in M.LN_CASES])
def test_layernorm(i, types):
    tin, tout = types
    for with_pe in (True, False):
        c, x, ref = M.ln_ref(i, tin, with_pe)
        name = "%s %s->%s pe%d" % (c.name, M.DT_ID[tin], M.DT_ID[tout], with_pe)
        buf, out = nan_out((c.rows, c.C), tout)
        y = ops().layernorm(dev_view(x.x), dev_view(x.gamma, float("nan")), dev_view(x.beta, float("nan")), 1e-5,
                            pe=dev_view(x.pe, float("nan")) if with_pe else None, out=out)
        guards_intact(buf, name)
        bound = M.ln_bound(ref, x.gamma, tout, c.L)
        print("RATIO layernorm rows/wave %d %-24s %s->%s pe%d L %2d  worst |err| / bound %.3f"
              % (c.rpw, c.name, M.DT_ID[tin], M.DT_ID[tout], with_pe, c.L, ratio(y.cpu(), ref.y, bound)))
        M.assert_within(name, y.cpu(), ref.y, bound)


# ------------------------------------------------------------------------------------------------ the plans' workspaces
GUARD = 4096             # bytes behind the workspace, filled with 0xA5


def test_launches_stay_inside_the_workspace_their_plan_states():
    """The launch is handed exactly the plan's workspace_bytes with a filled guard band behind: the band is untouched, the results equal
    those of a call with a generous workspace bit for bit, and a workspace one byte short is PF_ERR_ARG `workspace too small` before
    anything is launched (the outputs keep their NaN fill).  The smallest two-stage statistics case; a backward whose pixels per chunk
    have halved to 8, and its parameter gradients."""
    import ctypes as C

    from panfusion_amd import _lib
    o, lib = ops(), _lib.lib()
    p, st = o._p, o._stream

    def thrice(name, nbytes, outputs, launch):
        """launch(workspace pointer, bytes) -> status, run with a generous, the exact and a short workspace."""
        results = []
        for extra in (1 << 20, 0):
            ws = torch.full((nbytes + extra + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
            for t in outputs:
                t.fill_(float("nan"))
            assert launch(p(ws), nbytes + extra) == 0, (name, lib.pf_last_error_string())
            torch.cuda.synchronize()
            assert bool((ws[nbytes + extra:] == 0xA5).all()), "%s: wrote behind its workspace of %d bytes" % (name, nbytes + extra)
            assert all(bool(torch.isfinite(t).all()) for t in outputs), name
            results.append([t.clone() for t in outputs])
        for a, b in zip(*results):
            assert bool((bits(a) == bits(b)).all()), "%s: the exact workspace changes the result" % name
        for t in outputs:
            t.fill_(float("nan"))
        assert launch(p(ws), nbytes - 1) == 1 and (b"%s: workspace too small" % name.encode()) in lib.pf_last_error_string()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outputs), "%s: launched with a short workspace" % name

    # ---- statistics: n = 1, hw = 4099, C = 320, fp16 (two-stage, 17 pixels per chunk, a ragged last chunk)
    c = next(k for k in M.GN_CASES if k.name == "two_stage-1x4099x320-g32")
    x = M.gn_inputs(c, torch.float16, seed=11)
    g = _lib.GnPlan()
    assert lib.pf_groupnorm_plan(c.n, c.hw, c.c0, 0, c.groups, _lib.PF_F16, 0, 0, C.byref(g)) == 0
    assert (g.arm, g.ppc, g.nchunks) == (_lib.PF_GN_TWO_STAGE, 17, 242) and g.workspace_bytes == 242 * 512
    x0, gam, bet = dev_view(x.x0), x.gamma.to(DEV), x.beta.to(DEV)
    sc, sh = torch.empty(c.n, c.c0, device=DEV), torch.empty(c.n, c.c0, device=DEV)
    thrice("pf_groupnorm_stats", g.workspace_bytes, (sc, sh),
           lambda ws, nb: lib.pf_groupnorm_stats(p(x0), c.c0, None, 0, _lib.PF_F16, c.n, c.hw, c.groups, 1e-5, p(gam), p(bet), p(sc), p(sh), ws, nb, st()))
    # ---- backward and parameter gradients: n = 2, hw = 130, C = 64, 32 groups (17 chunks of 8 pixels, the last of 2), fp32 dy
    n, hw, Cc, groups = 2, 130, 64, 32
    b = _lib.GnBwdPlan()
    assert lib.pf_groupnorm_bwd_plan(n, hw, Cc, 0, groups, C.byref(b)) == 0 and (b.ppc, b.chunks) == (8, 17)
    gen = torch.Generator().manual_seed(77)
    xb = dev_view((torch.randn(n, hw, Cc, generator=gen) * 2 + 0.5).half())
    dy = dev_view(torch.randn(n, hw, Cc, generator=gen))
    gam, bet = (torch.randn(Cc, generator=gen) * 0.2 + 1).to(DEV), (torch.randn(Cc, generator=gen) * 0.1).to(DEV)
    sc, sh = o.groupnorm_scale_shift(xb, None, n, hw, groups, 1e-5, gam, bet)
    usc, ush = o.groupnorm_scale_shift(xb, None, n, hw, groups, 1e-5, torch.ones_like(gam), torch.zeros_like(bet))
    dx = torch.empty(n, hw, Cc, device=DEV)
    thrice("pf_groupnorm_bwd", b.bwd_workspace_bytes, (dx,),
           lambda ws, nb: lib.pf_groupnorm_bwd(p(xb), Cc, None, 0, _lib.PF_F16, n, hw, groups, 1e-5, p(gam), p(sc), p(sh), 1, p(dy), None,
                                               p(dx), None, ws, nb, st()))
    dgb = torch.empty(2 * Cc, device=DEV)
    thrice("pf_groupnorm_param_grads", b.param_workspace_bytes, (dgb,),
           lambda ws, nb: lib.pf_groupnorm_param_grads(p(xb), Cc, None, 0, _lib.PF_F16, n, hw, p(sc), p(sh), p(usc), p(ush), 1, p(dy), p(dgb),
                                                       ws, nb, st()))
