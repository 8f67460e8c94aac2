"""Float64 references, derived per-element error bounds, a summation-order emulation and the case tables for the
normalisation kernels of pf_elementwise.hip: the three producers of GroupNorm statistics (k_gn_stats_direct, k_gn_partial +
k_gn_finalize, k_gn_finalize_cols), the apply kernel k_scale_shift_act and k_layernorm.  A helper module: no tests in it, numpy
and torch on the CPU only.  It shares no code with the library: the host dispatch rules below are restated from its description.

Why: one rel-L2 over the tensor on inputs with E[x^2] ~ sigma^2 sees neither the conditioning of var = Q/n - mean^2 (the sums
are fp32 chains; the fp64 part only starts after them) nor a local defect (a dropped pixel of a ragged chunk moves rstd by 1e-4).

Notation.  u = 2^-24 (unit roundoff of fp32).  Per (image, group): mu, var (sigma^2), mabs = mean|x|, ex2 = E[x^2],
kappa = ex2 / (var + eps); with a circular wrap of p columns all of them are those of the explicitly padded tensor.
eps is the fp32 value of 1e-5 (what the kernels are handed), in every reference here.

L, the longest fp32 accumulation chain of an arm (every addition after it is fp64):
    direct     L = ceil(hw cpg / 256) + 6         a thread's strided walk (its first add is exact, one rounding of x x instead),
                                                  then the 6 butterfly steps of the wave; the 4 waves are combined in fp64
    two-stage  L = ceil(ppc / pix_par) + pix_par cpg     a thread's pixels of the chunk per channel, then the serial walk over
                                                  the [pix_par][cpg] block of shared memory; chunks are combined in fp64
The wrap weight (1 or 2) is exact in both.

Statistics.  A sum of fp32 terms t_i along a chain of L roundings is off by at most L u sum|t_i| (first order; L u < 1e-4):
    |d mean| <= L u mabs                          (then one cast to fp32: + u |mu|)
    |d var|  <= 3 L u ex2                         (L u ex2 from Q / n, 2 |mu| |d mean| <= 2 L u mabs^2 <= 2 L u ex2 from mean^2)
    |d rstd| / rstd <= 1.5 L u kappa + u          (rstd = (var + eps)^-1/2: half the relative error of var + eps, one cast)
The last line is first order in 3 L u kappa.  rstd_interval keeps the exact form -- rstd of var -+ |d var|, var clamped at 0 as
the kernels clamp it -- because a constant group has kappa = mu^2 / eps ~ 1e7 and the first-order form says nothing there;
test_norm_bounds_cpu.py checks that the two agree to 1e-3 where 3 L u kappa < 1e-3.  With rho that relative bound on rstd:
    scale = fl(rstd gamma)                |d scale| <= |scale| (rho + u)
    shift = fl(beta - fl(mean scale))     |d shift| <= dP + u (P + dP) + u (|beta| + P + dP),   P = |mu scale|,
                                          dP = |d mean| |scale| + |mu| |d scale| + |d mean| |d scale|
(an fma in place of the two roundings of shift is inside the same bound).

pf_groupnorm_from_partials.  The reference is float64 over the SAME fp32 partials; the kernel adds them in fp64 (an error of
ppi 2^-53 kappa, carried as PART_F64), so what is left is: mean cast (u), rstd cast (u), scale = fl(rstd gamma) (u), the product
and the difference of shift (u each):  |d scale| <= 2 u |scale|,  |d shift| <= 4 u |mu scale| + u |shift|.  kappa does not enter.

Apply.  The reference is float64 act(x sc + sh) with the scale / shift the GPU produced.  r = fma(x, sc, sh) is one rounding:
|d r| <= u A, A = |x sc| + |sh|.  SiLU is r * v_rcp(1 + v_exp(-r log2 e)): the argument product and the fp32 constant move
exp's argument by 2 u |r| (that much relative error of e^-r), v_exp and v_rcp are taken at 2 ulp = 4 u each (the kernel's comment
says 1-2 ulp), the sum and the product round once each.  An error of e^-r enters sigma(r) scaled by (1 - sigma):
    |d y32| <= |silu'(r)| u A + |y| ((4 u + 2 u |r|) (1 - sigma) + u + 4 u + u),   silu'(r) = sigma (1 + r (1 - sigma))
without SiLU |d y32| <= u A; with scale = None r = x exactly.  A 16-bit output adds one rounding, u16 (|y| + |d y32|), u16 = 2^-8
(bf16) or 2^-11 (fp16, + 2^-25 below the normal range).  The split pair and the raw pair are not bounded but pinned:
hi == round16(y32), lo == round16(y32 - hi) bit for bit, y32 the fp32 output of the same inputs.
End to end, against float64 GroupNorm(+SiLU) of the inputs: the apply bound + 1.1 (|x| |d scale| + |d shift|) (|silu'| <= 1.1).

LayerNorm.  v = fl(x + pe[row % pe_rows]) is ONE IEEE fp32 addition, the same on any machine: the reference takes v as its input
(computed in fp32 on the CPU), so that no input-magnitude term enters.  The kernel is two-pass; L = 8 KMAX + 6 (a lane's 8 KMAX
elements, 6 butterfly steps; the division by C is the rounding the exact first add leaves free), KMAX = 4 (one row per wave)
or 1 (four rows per wave):
    |d mean| <= L u mean|v|
    q = sum fl(fl(v - mean')^2):  sum (v - mean')^2 = C (var + d mean^2)  (the cross term vanishes: that is what two passes buy);
        relative error of q <= (L + 2) u, of q / C + eps 2 u more, sqrtf and the division at most 2 u each
    rho = (0.5 L + 6) u + 0.5 d mean^2 / (var + eps)         (second order in u; kappa does not appear)
    |d y32| <= |gamma| rstd |d mean| + |gamma| rstd |v - mu| (rho + 3 u) + u |y|      (v - mean', * rstd, * gamma, + beta)
    |d y|   <= |d y32| + u16 (|y| + |d y32|)
A one-pass variance q / C - mean^2 is off by L u E[v^2] / var instead: 2.3 at the rows offset by +1000.  It must fail, and does.

Every bound carries a factor SLACK = 1.01 for the second-order terms dropped above.

Emulation.  emulate_direct / emulate_two_stage / emulate_layernorm state the kernels' summation ORDER in numpy: sequential
fp32 inside a thread, the xor butterfly inside a wave, fp64 afterwards.  The compiler may contract q += f * f into an fma where
no wrap weight stands between (the file is built with contraction on); both forms are run (fma=False / True) and the maxima
below are over both.  Beside the hard bound a cap is set on what remains of the relative error of scale after its two final
roundings, per (image, group), in units of kappa u:
    excess = max(|d scale| / |scale| - 2 u, 0) / (kappa u)             cap = 2 x the emulation's maximum over the case table
Observed maxima of the emulation (test_norm_bounds_cpu.py::test_recorded_model_maxima re-measures them):
    direct     1.601 (1 x 1 x 64 fp32, kappa 9e5; 1.25 at 64 x 2560 fp16, kappa 9e4)   -> CAP["direct"]    = 3.20
    two_stage  3.168 (40 x 1024 x 128 fp16, kappa 9e4; 2.95 at L = 513)                -> CAP["two_stage"] = 6.34
    partials   |d scale| / (u |scale|) 1.953 of the derived 2, |d shift| / bound 0.944
    layernorm  |d y| / bound 0.987 (the output rounding alone reaches 1 / SLACK just above a power of two)
The typical excess is 0.2 - 1.0; the maxima above are over 1600 (image, group) pairs, and at mu >> sigma the roundings of a
chain are not independent.  On an MI355X the kernels give the same maxima to the printed digits.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U32 = 2.0 ** -24
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
SUBN16 = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 0.0}
EPS = float(np.float32(1e-5))
SLACK = 1.01
EXP_ULP = RCP_ULP = 2                      # v_exp_f32 / v_rcp_f32: "1-2 ulp" (pf_elementwise.hip), 1 ulp = 2 u
SILU_LIP = 1.1                             # sup |silu'|
OLD_TOL = {torch.bfloat16: 4e-3, torch.float16: 6e-4}       # TOL of tests/test_gpu_kernels.py

MODEL_MAX = dict(direct=1.601, two_stage=3.168, partials_scale=1.953, partials_shift=0.944, layernorm=0.987)
CAP = dict(direct=3.20, two_stage=6.34)

LADDER = (0.0, 3.0, 30.0, 300.0)           # mu / sigma of a group: kappa ~ 1, 10, 900, 90000
SIGMAS = (0.5, 1.0, 2.0)
CONST_MU = 10.0
OUTLIER = 64.0


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ host dispatch, restated
def gn_ppc(n, hw):
    """Pixels per statistics chunk of the two-stage arm."""
    ppc = max(8, min(64, n * hw // 2048))
    return min(hw, max(ppc, cdiv(hw, 256)))


def gn_arm(n, hw, C, groups):
    return "direct" if hw * (C // groups) <= 32768 and n * hw * C <= (4 << 20) else "two_stage"


def gn_pix_par(C):
    return 256 // min(C // 8, 256)


def gn_chain(n, hw, C, groups):
    """(arm, L) of a GroupNorm statistics call."""
    cpg = C // groups
    if gn_arm(n, hw, C, groups) == "direct":
        return "direct", cdiv(hw * cpg, 256) + 6
    pp = gn_pix_par(C)
    return "two_stage", cdiv(gn_ppc(n, hw), pp) + pp * cpg


def partials_gpb(hw, rows0, rows1, C, groups):
    ppi = max(hw // rows0, hw // rows1)
    gpb = 8 if ppi <= 32 else 4 if ppi <= 128 else 2 if ppi <= 512 else 1
    while gpb > 1 and gpb * (C // groups) // 2 > 512:
        gpb >>= 1
    return gpb


def partials_usable(hw, rows0, rows1, c0, C, groups):
    """Even channels per group and source, images that are whole runs of both sources, and at most 512 column pairs in one group (what
    a block of k_gn_finalize_cols holds at one group per block)."""
    return (C // groups) % 2 == 0 and c0 % 2 == 0 and hw % rows0 == 0 and hw % rows1 == 0 and (C // groups) // 2 <= 512


def ln_rows_per_wave(rows, C):
    return 4 if C <= 512 and rows >= 4096 else 1


# ------------------------------------------------------------------------------------------------ float64 references
def pad_circular(x, w, p):
    """[n, h*w, C] -> [n, h*(w+2p), C]: the width padded circularly by p columns, built explicitly."""
    n, hw, C = x.shape
    x4 = x.reshape(n, hw // w, w, C)
    return torch.cat([x4[:, :, w - p:], x4, x4[:, :, :p]], 2).reshape(n, -1, C)


def gn_reference(x, groups, gamma, beta, wrap=None, eps=EPS):
    """x [n, hw, C] (any float type, CPU; the channel concat of the sources).  Float64 moments per (image, group) -- of the tensor
    padded circularly by wrap = (w, p) when given -- and scale / shift [n, C] folded with gamma / beta."""
    x = x.double()
    if wrap is not None and wrap[1] > 0:
        x = pad_circular(x, *wrap)
    n, hw, C = x.shape
    xg = x.reshape(n, hw, groups, C // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
    mu, ex2, mabs = xg.mean(-1), (xg * xg).mean(-1), xg.abs().mean(-1)
    var = ((xg - mu[..., None]) ** 2).mean(-1)
    rstd = (var + eps).rsqrt()
    per_c = lambda t: t.repeat_interleave(C // groups, 1)
    scale = per_c(rstd) * gamma.double()
    shift = beta.double() - per_c(mu) * scale
    return SimpleNamespace(mu=mu, var=var, mabs=mabs, ex2=ex2, rstd=rstd, kappa=ex2 / (var + eps), scale=scale, shift=shift,
                           groups=groups, C=C, per_c=per_c)


def silu64(r):
    return r * torch.sigmoid(r)


def apply_reference(x, scale, shift, act):
    """float64 act(x * scale + shift), x [n, hw, C], scale / shift [n, C] or None."""
    r = x.double()
    if scale is not None:
        r = r * scale.double()[:, None] + shift.double()[:, None]
    return silu64(r) if act else r


def ln_input(x, pe):
    """v = fl32(x + pe[row % pe_rows]): the kernel's ONE fp32 addition, done in fp32 here as well (see the docstring)."""
    v = x.float()
    if pe is not None:
        v = v + pe.float()[torch.arange(x.shape[0]) % pe.shape[0]]
    return v


def ln_reference(x, pe, gamma, beta, eps=EPS):
    v = ln_input(x, pe).double()
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = (v - mu) * rstd * gamma.double() + beta.double()
    return SimpleNamespace(v=v, mu=mu, var=var, rstd=rstd, y=y, mabs=v.abs().mean(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------ bounds
def rstd_first_order(ref, L):
    return 1.5 * L * U32 * ref.kappa + U32


def rstd_interval(ref, L, eps=EPS):
    """Relative bound on rstd [n, groups]: exact in |d var| <= 3 L u ex2 with the clamp at var = 0, plus the cast."""
    D = 3 * L * U32 * ref.ex2
    hi = ((ref.var - D).clamp_min(0) + eps).rsqrt()
    lo = (ref.var + D + eps).rsqrt()
    return torch.maximum(hi / ref.rstd - 1, 1 - lo / ref.rstd) + U32


def gn_stat_bounds(ref, L, gamma, beta):
    """(bound on |d scale|, bound on |d shift|) [n, C] of a statistics producer with chain length L."""
    rho = ref.per_c(rstd_interval(ref, L))
    dm = ref.per_c(L * U32 * ref.mabs + U32 * ref.mu.abs())
    mu = ref.per_c(ref.mu).abs()
    S = ref.scale.abs()
    dS = S * (rho + U32)
    P = mu * S
    dP = dm * S + mu * dS + dm * dS
    dH = dP + U32 * (P + dP) + U32 * (beta.double().abs() + P + dP)
    return SLACK * dS, SLACK * dH


def partials_bounds(ref, ppi, beta):
    f64 = 2.0 ** -52 * (ppi + 8) * ref.per_c(ref.kappa)
    S, P = ref.scale.abs(), (ref.per_c(ref.mu) * ref.scale).abs()
    return SLACK * (2 * U32 + f64) * S, SLACK * ((4 * U32 + f64) * P + U32 * ref.shift.abs())


def apply_bound(x, scale, shift, act, out_dtype):
    """(float64 reference, per-element bound) of k_scale_shift_act with THESE scale / shift (fp32, as the GPU produced them)."""
    x = x.double()
    if scale is not None:
        xs = x * scale.double()[:, None]
        r = xs + shift.double()[:, None]
        dr = U32 * (xs.abs() + shift.double().abs()[:, None])
    else:
        r, dr = x, torch.zeros_like(x)
    if act:
        sg = torch.sigmoid(r)
        y = r * sg
        rel = (EXP_ULP * 2 * U32 + 2 * U32 * r.abs()) * (1 - sg) + U32 + RCP_ULP * 2 * U32 + U32
        b32 = (sg * (1 + r * (1 - sg))).abs() * dr + dr * dr + y.abs() * rel + 1e-37
    else:
        y, b32 = r, dr
    b = b32 + U16[out_dtype] * (y.abs() + b32) + SUBN16[out_dtype]
    return y, SLACK * b


def gn_end_to_end_bound(x, ref, got_scale, got_shift, dscale, dshift, act, out_dtype):
    """(float64 GroupNorm(+SiLU) of x, bound): the apply bound with the produced scale / shift + the statistics bound carried
    through the affine map."""
    _, b = apply_bound(x, got_scale, got_shift, act, out_dtype)
    y = apply_reference(x, ref.scale, ref.shift, act)
    carry = (SILU_LIP if act else 1.0) * (x.double().abs() * dscale[:, None] + dshift[:, None])
    return y, b + (1 + U16[out_dtype]) * carry


def ln_chain(rows, C):
    return 8 * (1 if ln_rows_per_wave(rows, C) == 4 else 4) + 6


def ln_bound(ref, gamma, out_dtype, L, eps=EPS):
    g = gamma.double().abs()
    dm = L * U32 * ref.mabs
    rho = (0.5 * L + 6) * U32 + 0.5 * dm * dm / (ref.var + eps)
    b32 = g * ref.rstd * dm + g * ref.rstd * (ref.v - ref.mu).abs() * (rho + 3 * U32) + U32 * ref.y.abs()
    return SLACK * (b32 + U16[out_dtype] * (ref.y.abs() + b32) + SUBN16[out_dtype])


def excess_ratio(got_scale, ref):
    """[n, groups]: worst over a group's channels of max(|d scale| / |scale| - 2 u, 0) / (kappa u)."""
    rel = (got_scale.double() - ref.scale).abs() / ref.scale.abs().clamp_min(1e-300)
    n, C = rel.shape
    rel = rel.reshape(n, ref.groups, C // ref.groups).amax(-1)
    return (rel - 2 * U32).clamp_min(0) / (ref.kappa * U32)


def worst(err, bound):
    return float((err / bound.clamp_min(1e-300)).max())


def assert_within(name, got, want, bound):
    """|got - want| <= bound for every element; a failure names the worst element, its ratio and how many exceed."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), "%s: non-finite output" % name
    err = (got - want).abs()
    bad = int((err > bound).sum())
    if bad:
        ratio = err / bound.clamp_min(1e-300)
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(want.shape)))
        raise AssertionError("%s: %d of %d elements exceed the bound; worst at %s: got %.9g, want %.9g, |err| %.3e = %.2f x bound %.3e"
                             % (name, bad, err.numel(), idx, float(got.flatten()[i]), float(want.flatten()[i]),
                                float(err.flatten()[i]), float(ratio.flatten()[i]), float(bound.flatten()[i])))
    return worst(err, bound)


def assert_cap(name, got_scale, ref, arm):
    r = excess_ratio(got_scale, ref)
    bad = int((r > CAP[arm]).sum())
    if bad:
        i = int(r.argmax())
        raise AssertionError("%s: %d of %d (image, group) exceed the cap; worst at %s: (|d scale| / |scale| - 2u) / (kappa u) = %.3f > %.2f "
                             "(kappa %.3g)" % (name, bad, r.numel(), (i // ref.groups, i % ref.groups), float(r.flatten()[i]),
                                               CAP[arm], float(ref.kappa.flatten()[i])))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ emulation
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _seq(a, axis):
    """Sequential fp32 sum along `axis` (np.cumsum adds one element at a time in the accumulator's type)."""
    return np.cumsum(_f32(a), axis=axis, dtype=np.float32).take(-1, axis=axis)


def _seq_sq(a, axis, fma):
    """Sequential fp32 sum of squares: q = fl(q + fl(a a)), or q = fma(a, a, q) (the product of two fp32 is exact in fp64)."""
    a = _f32(a)
    if not fma:
        return _seq(a * a, axis)
    a = np.moveaxis(a, axis, 0)
    q = np.zeros(a.shape[1:], np.float32)
    for k in range(a.shape[0]):
        q = (q.astype(np.float64) + a[k].astype(np.float64) ** 2).astype(np.float32)
    return q


def _butterfly(v):
    """v += shfl_xor(v, o), o = 32 .. 1, over the last axis (64 lanes), fp32; every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def wrap_weights(hw, wrap, defect=None):
    wt = np.ones(hw, np.float32)
    if wrap is not None and wrap[1] > 0:
        w, p = wrap
        col = np.arange(hw) % w
        wt[((col <= p) if defect == "wrap_le" else (col < p)) | (col >= w - p)] = 2.0
    return wt


def _finish(S, Q, cnt, gamma, beta, cpg, fma, eps=EPS):
    """fp64 moments -> fp32 mean / rstd -> fp32 scale / shift [n, C], as the tail of all three producers."""
    mean = S / cnt
    var = np.maximum(Q / cnt - mean * mean, 0.0)
    m32 = np.repeat(_f32(mean), cpg, 1)
    r32 = np.repeat(_f32(1.0 / np.sqrt(var + eps)), cpg, 1)
    g, b = _f32(gamma.numpy()), _f32(beta.numpy())
    sc = r32 * g
    if fma:
        sh = (b.astype(np.float64) - m32.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    else:
        sh = b - m32 * sc
    return torch.from_numpy(sc), torch.from_numpy(sh)


def concat_sources(x0, x1, defect=None):
    """The channel concat the kernels read.  defect 'src_offset': the second source addressed with c, not c - c0."""
    if x1 is None:
        return x0.float()
    if defect == "src_offset":
        n, hw, c1 = x1.shape
        c0 = x0.shape[-1]
        flat = x1.float().flatten()
        idx = (torch.arange(n * hw)[:, None] * c1 + c0 + torch.arange(c1)[None]) % flat.numel()
        x1 = flat[idx].reshape(n, hw, c1)
    return torch.cat([x0.float(), x1.float()], -1)


def emulate_direct(x, groups, gamma, beta, wrap=None, fma=False, defect=None):
    """k_gn_stats_direct: thread t of 256 adds elements t, t + 256, .. of the group's [hw][cpg] block."""
    x = _f32(x.numpy())
    n, hw, C = x.shape
    cpg = C // groups
    wt = np.repeat(wrap_weights(hw, wrap, defect), cpg)
    xg = x.reshape(n, hw, groups, cpg).transpose(0, 2, 1, 3).reshape(n, groups, hw * cpg)
    Lc = cdiv(hw * cpg, 256)
    f = np.zeros((n, groups, Lc * 256), np.float32)
    f[..., :hw * cpg] = xg
    ww = np.ones(Lc * 256, np.float32)
    ww[:hw * cpg] = wt
    f, ww = f.reshape(n, groups, Lc, 256), ww.reshape(Lc, 256)
    s = _seq(f * ww, 2)
    q = _seq_sq(f, 2, True) if fma and wrap is None else _seq(f * f * ww, 2)
    S = _butterfly(s.reshape(n, groups, 4, 64)).astype(np.float64).sum(-1)
    Q = _butterfly(q.reshape(n, groups, 4, 64)).astype(np.float64).sum(-1)
    counted = hw if wrap is None or defect == "hw_counted" else hw // wrap[0] * (wrap[0] + 2 * wrap[1])
    return _finish(S, Q, float(counted) * cpg, gamma, beta, cpg, fma)


def emulate_two_stage(x, groups, gamma, beta, wrap=None, fma=False, defect=None):
    """k_gn_partial + k_gn_finalize: per chunk of ppc pixels, slot s of pix_par adds pixels s, s + pix_par, .. per channel;
    one thread per group then walks [pix_par][cpg] serially; the chunks meet in fp64."""
    x = _f32(x.numpy())
    n, hw, C = x.shape
    cpg = C // groups
    ppc, pp = gn_ppc(n, hw), gn_pix_par(C)
    nch, K = cdiv(hw, ppc), cdiv(ppc, pp)
    wt = wrap_weights(hw, wrap, defect)
    if defect == "drop_last_pixel":
        x = x.copy()
        x[:, hw - 1] = 0
    xp = np.zeros((n, nch, K * pp, C), np.float32)
    wp = np.ones((nch, K * pp), np.float32)
    for ch in range(nch):                                   # (the ragged last chunk and the slots' tails stay zero: exact adds)
        a, b = ch * ppc, min(hw, (ch + 1) * ppc)
        xp[:, ch, :b - a] = x[:, a:b]
        wp[ch, :b - a] = wt[a:b]
    xp = xp.reshape(n, nch, K, pp, C)
    wp = wp.reshape(1, nch, K, pp, 1)
    s = _seq(xp * wp, 2)
    q = _seq_sq(xp, 2, True) if fma and wrap is None else _seq(xp * xp * wp, 2)
    walk = lambda t: _seq(t.reshape(n, nch, pp, groups, cpg).transpose(0, 1, 3, 2, 4).reshape(n, nch, groups, pp * cpg), 3)
    s, q = walk(s).astype(np.float64), walk(q).astype(np.float64)
    S, Q = s.sum(1), q.sum(1)
    if defect == "chunk_twice":
        S, Q = S + s[:, nch // 2], Q + q[:, nch // 2]
    counted = hw if wrap is None or defect == "hw_counted" else hw // wrap[0] * (wrap[0] + 2 * wrap[1])
    return _finish(S, Q, float(counted) * cpg, gamma, beta, cpg, fma)


def emulate_groupnorm(x, groups, gamma, beta, wrap=None, fma=False, defect=None):
    n, hw, C = x.shape
    f = emulate_direct if gn_arm(n, hw, C, groups) == "direct" else emulate_two_stage
    return f(x, groups, gamma, beta, wrap, fma, defect)


def make_partials(x, rows):
    """[n, hw, c] -> the column-pair moments a GEMM epilogue leaves: fp32 [n * hw / rows][2][c / 2] (sum, sum of squares of
    columns (2k, 2k + 1) over runs of `rows` rows)."""
    n, hw, c = x.shape
    r = x.double().reshape(n * hw // rows, rows, c // 2, 2)
    return torch.stack([r.sum((1, 3)), (r * r).sum((1, 3))], 1).float().contiguous()


def partials_reference(parts, cs, n, hw, groups, gamma, beta, eps=EPS):
    """float64 GroupNorm moments from the fp32 partials themselves: parts[i] [n * ppi_i][2][cs[i] / 2]."""
    cols = [p.double().reshape(n, -1, 2, c // 2).sum(1) for p, c in zip(parts, cs)]
    col = torch.cat(cols, -1)                               # [n, 2, C / 2]
    C = sum(cs)
    cpg = C // groups
    g = col.reshape(n, 2, groups, cpg // 2).sum(-1)
    cnt = float(hw) * cpg
    mu, ex2 = g[:, 0] / cnt, g[:, 1] / cnt
    var = (ex2 - mu * mu).clamp_min(0)
    rstd = (var + eps).rsqrt()
    per_c = lambda t: t.repeat_interleave(cpg, 1)
    scale = per_c(rstd) * gamma.double()
    return SimpleNamespace(mu=mu, var=var, ex2=ex2, rstd=rstd, kappa=ex2 / (var + eps), scale=scale,
                           shift=beta.double() - per_c(mu) * scale, groups=groups, C=C, per_c=per_c)


def emulate_partials(parts, cs, n, hw, groups, gamma, beta, fma=False):
    """k_gn_finalize_cols: fp64 sums of the partials, then the common tail."""
    ref = partials_reference(parts, cs, n, hw, groups, gamma, beta)
    cnt = float(hw) * (ref.C // groups)
    return _finish(ref.mu.numpy() * cnt, ref.ex2.numpy() * cnt, cnt, gamma, beta, ref.C // groups, fma)


def emulate_layernorm(x, pe, gamma, beta, out_dtype, fma=False, defect=None, eps=EPS):
    """k_layernorm: lane l of 64 holds octets l, l + 64, ..; mean and the centred sum of squares are a lane's serial fp32 sum,
    the butterfly, one division.  Defects: 'one_pass' (var = q / C - mean^2), 'pe_mod' (pe row taken modulo pe_rows + 1),
    'skip_last_row' (the last row of every 4-row group left unwritten: zeros)."""
    rows, C = x.shape
    if defect == "pe_mod":
        v = x.float() + torch.cat([pe, pe[:1]]).float()[torch.arange(rows) % (pe.shape[0] + 1)]
    else:
        v = ln_input(x, pe)
    v = _f32(v.numpy())
    K = cdiv(C // 8, 64)
    lanes = np.zeros((rows, K, 64, 8), np.float32)
    lanes.reshape(rows, -1)[:, :C] = v
    lanes = lanes.transpose(0, 2, 1, 3).reshape(rows, 64, K * 8)            # a lane's elements in the order it adds them
    live = np.zeros((1, K, 64, 8), bool)
    live.reshape(1, -1)[:, :C] = True
    live = live.transpose(0, 2, 1, 3).reshape(1, 64, K * 8)
    Cf = np.float32(C)
    mean = (_butterfly(_seq(lanes, 2)) / Cf).astype(np.float32)
    if defect == "one_pass":
        var = (_butterfly(_seq_sq(lanes, 2, fma)) / Cf).astype(np.float32) - mean * mean
        var = np.maximum(var, np.float32(0))
    else:
        d = np.where(live, lanes - mean[:, None, None], np.float32(0))
        var = (_butterfly(_seq_sq(d, 2, fma)) / Cf).astype(np.float32)
    rstd = (np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)).astype(np.float32)
    t = (v - mean[:, None]) * rstd[:, None]
    g, b = _f32(gamma.numpy()), _f32(beta.numpy())
    y = (t.astype(np.float64) * g + b).astype(np.float32) if fma else t * g + b
    y = torch.from_numpy(y).to(out_dtype)
    if defect == "skip_last_row":
        y[3::4] = 0
    return y


# ------------------------------------------------------------------------------------------------ inputs
def ladder_tensor(n, hw, C, groups, gen, const_group=True):
    """fp32 [n, hw, C]: group g of image i has sigma = SIGMAS[g % 3] and mu / sigma = LADDER[(g + i) % 4] (neighbouring groups of
    one image differ by orders of magnitude in kappa); one group of image 0 is the constant CONST_MU."""
    cpg = C // groups
    g = torch.arange(groups)
    sig = torch.tensor(SIGMAS)[g % 3]
    x = torch.randn(n, hw, C, generator=gen)
    for i in range(n):
        ratio = torch.tensor(LADDER)[(g + i) % 4]
        x[i] = x[i] * sig.repeat_interleave(cpg) + (ratio * sig).repeat_interleave(cpg)
    if const_group:
        cg = const_group_of(groups)
        x[0, :, cg * cpg:(cg + 1) * cpg] = CONST_MU
    return x, sig.repeat_interleave(cpg)


def const_group_of(groups):
    return 5 if groups > 5 else 1


def outlier_sites(hw, c0, c1, groups, wrap):
    """(pixel, channel) of the one-hot outliers: the last pixel (of the last, ragged chunk) at the last channel of the last source
    and at the first channel after the source boundary; with a wrap the four columns at the edges of the doubled bands."""
    C = c0 + c1
    cpg = C // groups
    sites = [(hw - 1, C - 1)]
    if c1:
        sites += [(hw - 1, c0), (0, c0 - 1)]
    if wrap is not None:
        w, p = wrap
        row = hw // w - 1
        cg = const_group_of(groups)
        chans = [c for c in range(0, C, cpg) if c // cpg != cg]
        for k, col in enumerate(sorted({p - 1, p, w - p - 1, w - p})):
            sites.append((row * w + col, chans[(2 + 3 * k) % len(chans)]))
    return sites


def gn_inputs(c, dtype, seed=0):
    """Seeded inputs of a GroupNorm case rounded to `dtype` (CPU): x0 [n, hw, c0], x1 [n, hw, c1] or None, gamma, beta fp32."""
    gen = torch.Generator().manual_seed(2000 + seed)
    C = c.c0 + c.c1
    x, sig = ladder_tensor(c.n, c.hw, C, c.groups, gen)
    for (p, ch) in outlier_sites(c.hw, c.c0, c.c1, c.groups, c.wrap):
        x[:, p, ch] += OUTLIER * sig[ch]
    x = x.to(dtype)
    gamma = torch.randn(C, generator=gen) * 0.2 + 1
    beta = torch.randn(C, generator=gen) * 0.1
    x0 = x[..., :c.c0].contiguous()
    x1 = x[..., c.c0:].contiguous() if c.c1 else None
    return SimpleNamespace(x0=x0, x1=x1, x=x, gamma=gamma, beta=beta)


def plain_inputs(c, dtype, seed=0):
    """The inputs the rel-L2 tests of the suite use (randn * 2 + 0.5, kappa ~ 1), for the defect comparison."""
    gen = torch.Generator().manual_seed(3000 + seed)
    C = c.c0 + c.c1
    x = (torch.randn(c.n, c.hw, C, generator=gen) * 2 + 0.5).to(dtype)
    gamma = torch.randn(C, generator=gen) * 0.2 + 1
    beta = torch.randn(C, generator=gen) * 0.1
    return SimpleNamespace(x0=x[..., :c.c0].contiguous(), x1=x[..., c.c0:].contiguous() if c.c1 else None, x=x, gamma=gamma, beta=beta)


LN_OFFSET = 1000.0


def ln_offset_rows(rows):
    return sorted({0, rows // 2, rows - 1} if rows < 8 else {1, rows // 2, rows - 1})


def ln_inputs(c, dtype, seed=0):
    """x [rows, C] rounded to `dtype`, a few rows offset by +1000; pe fp32 [37, C]; gamma, beta."""
    gen = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(c.rows, c.C, generator=gen) + 0.3
    x[ln_offset_rows(c.rows)] += LN_OFFSET
    pe = torch.randn(LN_PE_ROWS, c.C, generator=gen)
    gamma = torch.randn(c.C, generator=gen) * 0.2 + 1
    beta = torch.randn(c.C, generator=gen) * 0.1
    return SimpleNamespace(x=x.to(dtype), pe=pe, gamma=gamma, beta=beta)


# ------------------------------------------------------------------------------------------------ case tables
F16S = (torch.bfloat16, torch.float16)
ALL3 = (torch.bfloat16, torch.float16, torch.float32)
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def gn_case(kind, n, hw, c0, c1, groups, wrap=None):
    C = c0 + c1
    arm, L = gn_chain(n, hw, C, groups)
    name = "%s-%dx%dx%d%s-g%d%s" % (kind, n, hw, c0, "+%d" % c1 if c1 else "", groups, "-wrap%dx%d" % wrap if wrap else "")
    return SimpleNamespace(kind=kind, name=name, n=n, hw=hw, c0=c0, c1=c1, groups=groups, wrap=wrap, arm=arm, L=L)


# (kind names the arm and how the shape reaches it; gn_case asserts nothing -- test_norm_bounds_cpu.py checks kind against arm)
GN_CASES = [
    # direct: hw cpg <= 32768 and n hw C <= 4 Mi
    gn_case("direct", 3, 17 * 24, 64, 32, 32), gn_case("direct", 1, 64, 1280, 1280, 32), gn_case("direct", 2, 1, 64, 0, 32),
    # two-stage through hw cpg: ragged last chunk with pix_par = 6 (16 idle threads); 65-pixel chunks over 32 slots; two `ob`
    # rounds (320 octets, pix_par = 1); two sources
    gn_case("two_stage", 1, 4099, 320, 0, 32), gn_case("two_stage", 1, 16411, 64, 0, 32), gn_case("two_stage", 1, 421, 2560, 0, 32),
    gn_case("two_stage", 2, 4096, 192, 128, 32),
    # two-stage through the element cap; the second has pix_par = 128 > ppc = 64 (slots that never see a pixel)
    gn_case("two_stage_cap", 40, 1024, 128, 0, 32), gn_case("two_stage_cap", 40, 8190, 16, 0, 4),
    # wrap: direct (the second doubles every column: 2 p == w), two-stage with chunks of 33 pixels (quarter rows of 132) and of
    # 34 (h = 65: chunks straddle the image rows)
    gn_case("direct", 2, 6 * 16, 64, 32, 32, wrap=(16, 2)), gn_case("direct", 1, 5 * 8, 64, 0, 32, wrap=(8, 4)),
    gn_case("two_stage", 1, 64 * 132, 320, 0, 32, wrap=(132, 2)), gn_case("two_stage", 1, 65 * 132, 320, 0, 32, wrap=(132, 2)),
]


def part_case(name, n, hw, c0, rows0, c1, rows1, groups):
    C = c0 + c1
    usable = partials_usable(hw, rows0, rows1 or rows0, c0, C, groups)
    gpb = partials_gpb(hw, rows0, rows1 or rows0, C, groups) if usable else 0
    npairs = min(gpb * (C // groups) // 2, C // 2)
    return SimpleNamespace(name=name, n=n, hw=hw, c0=c0, rows0=rows0, c1=c1, rows1=rows1 or rows0, groups=groups, usable=usable, gpb=gpb,
                           npairs=npairs, slices=(256 // npairs if npairs <= 128 else 1) if usable else 0, wrap=None)


PART_CASES = [
    part_case("gpb8-320pairs", 2, 64, 2560, 8, 0, 0, 32),              # slices = 1, two rounds of 256 pairs
    part_case("gpb8-160pairs", 2, 256, 1280, 16, 0, 0, 32),            # slices = 1, one round
    part_case("gpb4-ppi64", 2, 1024, 128, 16, 0, 0, 32),               # VAE-like: 2 pairs per group, 32 slices
    part_case("gpb2-ppi256", 2, 1024, 128, 4, 0, 0, 32),
    part_case("gpb1-ppi1024", 2, 1024, 128, 1, 0, 0, 32),
    part_case("two-sources", 2, 256, 192, 64, 128, 16, 32),            # ppi 4 and 16; 40 pairs -> 6 slices, 16 idle threads
    part_case("ragged-block", 2, 64, 96, 8, 0, 0, 12),                 # the second block holds 4 of gpb = 8 groups
    part_case("gpb-halved", 1, 64, 2560, 8, 0, 0, 8),                  # 160 pairs per group: gpb 8 -> 2
    part_case("refused-odd-cpg", 2, 64, 96, 8, 0, 0, 32),              # cpg = 3: the statistics pass
    part_case("refused-rows", 2, 100, 128, 8, 0, 0, 32),               # 100 % 8 != 0: the statistics pass
]

# (input type, output type, kind): kind 'plain' / 'split' / 'raw' (plain output + the raw pair)
APPLY_COMBOS = ([(t, t, k) for t in F16S for k in ("plain", "split")] + [(t, torch.float32, "plain") for t in ALL3] +
                [(torch.float32, t, k) for t in F16S for k in ("plain", "split", "raw")])
APPLY_SHAPES = {"plain": (2, 77, 64, 40), "split": (2, 77, 64, 32), "raw": (2, 77, 64, 32)}     # 13 octets x 77 pixels: odd per_img

LN_PE_ROWS = 37


def ln_case(rows, C):
    r = ln_rows_per_wave(rows, C)
    return SimpleNamespace(name="rows%d-%dx%d" % (r, rows, C), rows=rows, C=C, rpw=r, L=ln_chain(rows, C))


LN_CASES = ([ln_case(r, C) for r in (4096, 4099) for C in (8, 64, 320, 512)] +
            [ln_case(r, C) for r in (1, 37 * 3, 4097) for C in (8, 520, 1280, 2048)])
LN_TYPES = [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.float32, torch.bfloat16), (torch.float32, torch.float16)]


@functools.lru_cache(maxsize=4)
def gn_ref(i, dtype):
    """(case, inputs, float64 reference) of GN_CASES[i]; computed once and shared."""
    c = GN_CASES[i]
    x = gn_inputs(c, dtype, seed=i)
    return c, x, gn_reference(x.x, c.groups, x.gamma, x.beta, c.wrap)


@functools.lru_cache(maxsize=4)
def ln_ref(i, dtype, with_pe):
    c = LN_CASES[i]
    x = ln_inputs(c, dtype, seed=i)
    return c, x, ln_reference(x.x, x.pe if with_pe else None, x.gamma, x.beta)


def part_inputs(c, seed=0):
    """fp32 sources of a from-partials case (the kappa ladder without the constant group), gamma, beta."""
    gen = torch.Generator().manual_seed(5000 + seed)
    C = c.c0 + c.c1
    x, _ = ladder_tensor(c.n, c.hw, C, c.groups, gen, const_group=False)
    gamma = torch.randn(C, generator=gen) * 0.2 + 1
    beta = torch.randn(C, generator=gen) * 0.1
    x0 = x[..., :c.c0].contiguous()
    x1 = x[..., c.c0:].contiguous() if c.c1 else None
    return SimpleNamespace(x0=x0, x1=x1, x=x, gamma=gamma, beta=beta)
