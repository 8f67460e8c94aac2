"""Float64 reference, componentwise error bounds and a rounding model for the attention kernels
(pf_attention.hip, pf_backward.hip).  A helper module: no tests in it, torch on the CPU only.

Why: a rel-L2 over the whole output cannot see a local defect (one wrong query row of 12288 moves it by
1e-3), and the defects these kernels can have are local.  The checks here are per element and per row.

Reference.  ref_forward / ref_backward work in float64 on the already-rounded 16-bit inputs and also return the
MAGNITUDE products the bounds are made of (A = P |V| and friends): what the result would be without cancellation.

Bounds (u = unit roundoff of the storage type: 2^-8 for bf16, 2^-11 for fp16):

  forward, every arm      |got - O| <= 4u A + F
      1u  P is rounded to 16 bits before the second product (relative error u on the numerator)
      1u  the MSUM / ping-pong kernels take the denominator from the same rounded P
      1u  the output is rounded once: u |O| <= u A
          (split key range instead: P, each normalised partial output, the merged output -- 3u as well)
      1u  allowance for fp32 accumulation over nk terms, v_exp_f32 and fp32 score rounding (each orders below u)
  F   fp16 only: an entry of P whose unnormalised value p l (l = sum exp(s - max s) >= 1) is below 2^-14 may be
      flushed or lose bits as a subnormal; its error is at most its own contribution: F = (P o [P l < 2^-14]) |V|.
      The kernels' deferred rescale only RAISES unnormalised values (stale reference point), so this is conservative.
  backward  |dV err| <= 3u A_V + F_V,  |dQ err| <= 3u A_Q + 2^-20 C_Q + F_Q,  |dK err| <= 3u A_K + 2^-20 C_K + F_K
      P or dS rounded to 16 bits, the output rounded once, one u of allowance; the 2^-20 C term covers the fp32
      cancellation in dp - delta and in s - lse; F_* as F, from the entries of P / |dS| below 2^-14 (fp16 only).

Row check.  The componentwise bound is a worst case (three to five times the typical error), so a second statistic
is taken per (batch, head, row): the RMS over the head's channels of |err| / (u A), in fp16 |err| / (u A + F).  (F in
the denominator: a model that flushes the fp16 subnormals of P, which hardware may do, reaches 11 on |err| / (u A)
alone in a spiked row -- all of it inside F; tests/test_attention_bounds_cpu.py keeps the median of F / (u A) below
0.1 on every case so that F cannot hollow either check.)  The cap comes from the MODEL below, never from the GPU
kernels: twice the largest value the model produces over every case of FWD_CASES / BWD_CASES in both types, with the
fp16 subnormals of P and dS kept and flushed.

The model.  emulate_forward / emulate_backward state the kernels' rounding points in fp32 torch -- P to the 16-bit
type, fp32 accumulation, output to the 16-bit type; for a split key range per-split normalised 16-bit partial
outputs with an fp32 log-sum-exp and a weighted merge -- over an online softmax in key tiles with the deferred
rescale (the reference point of a 32-row group moves only when a row grew by more than 2^8).  Written from that
description: it shares no code with the library.

Observed maxima of the model over all cases, both types (they back the derived factors 4 and 3 and set the row caps;
test_attention_bounds_cpu.py::test_recorded_model_maxima re-measures them):
    forward   max |err| / (u A)    1.54  (split key range with a spike key, fp16; bound factor 4)
    backward  max |err| / (u A_*)  1.27  (bound factor 3)
    forward   max row RMS          0.722 -> ROW_CAP_FWD = 1.45
    backward  max row RMS          0.527 -> ROW_CAP_BWD = 1.06
"""
import functools
from types import SimpleNamespace

import torch

LOG2E = 1.4426950408889634
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FLUSH = 2.0 ** -14                     # smallest normal fp16
CANCEL = 2.0 ** -20                    # fp32 cancellation allowance of the backward (see the docstring)
OLD_TOL = {torch.bfloat16: 2.5 * 4e-3, torch.float16: 2.5 * 6e-4}      # what the rel-L2 tests of the suite accept

# model maxima (see the docstring) and the caps derived from them: cap = 2 x the model's largest row RMS, rounded up
MODEL_MAX = dict(FWD_ELEM=1.54, BWD_ELEM=1.27, FWD_ROW=0.722, BWD_ROW=0.527)
ROW_CAP_FWD = 1.45
ROW_CAP_BWD = 1.06


# ------------------------------------------------------------------------------------------------ layouts
def heads(x, H, dtype=torch.float64):
    """[B, n, H*D] -> [B, H, n, D] in `dtype`."""
    B, n, C = x.shape
    return x.to(dtype).reshape(B, n, H, C // H).transpose(1, 2)


def rows(x):
    """[B, H, n, D] -> [B, n, H*D]."""
    B, H, n, D = x.shape
    return x.transpose(1, 2).reshape(B, n, H * D)


# ------------------------------------------------------------------------------------------------ reference
def ref_forward(q, k, v, H, scale, bias=None):
    """float64 attention on 16-bit-valued q [B, nq, C], k / v [B, nk, C], bias [nq, nk] or None.
    O, A, F are [B, nq, C]; P, S [B, H, nq, nk]; lse (log2 domain) and l [B, H, nq]."""
    qh, kh, vh = heads(q, H), heads(k, H), heads(v, H)
    S = qh @ kh.transpose(-1, -2) * scale
    if bias is not None:
        S = S + bias.double()
    m = S.amax(-1, keepdim=True)
    E = torch.exp(S - m)
    l = E.sum(-1, keepdim=True)
    P = E / l
    va = vh.abs()
    F = rows((P * (E < FLUSH)) @ va)                   # P l = E
    return SimpleNamespace(O=rows(P @ vh), P=P, S=S, lse=((m + torch.log(l)) * LOG2E).squeeze(-1), A=rows(P @ va), F=F,
                           l=l.squeeze(-1))


def ref_backward(q, k, v, dout, H, scale, bias=None):
    """Closed-form float64 backward (not autograd): dP = dO V^T, delta = rowsum(O o dO), dS = P o (dP - delta),
    dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO, with the magnitude products of the bounds.  lse / delta [B, H, nq]."""
    f = ref_forward(q, k, v, H, scale, bias)
    qh, kh, vh, doh = heads(q, H), heads(k, H), heads(v, H), heads(dout, H)
    P = f.P
    dP = doh @ vh.transpose(-1, -2)
    delta = (heads(f.O, H) * doh).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    aS = dS.abs()
    cS = P * (dP.abs() + delta.abs())
    qa, ka, da = qh.abs(), kh.abs(), doh.abs()
    PT, aST = P.transpose(-1, -2), aS.transpose(-1, -2)
    smallP, smallS = P * (P < FLUSH), aS * (aS < FLUSH)
    return SimpleNamespace(
        O=f.O, P=P, dS=dS, lse=f.lse, delta=delta.squeeze(-1),
        dQ=rows(dS @ kh) * scale, dK=rows(dS.transpose(-1, -2) @ qh) * scale, dV=rows(PT @ doh),
        A_V=rows(PT @ da), A_Q=rows(aS @ ka) * scale, A_K=rows(aST @ qa) * scale,
        C_Q=rows(cS @ ka) * scale, C_K=rows(cS.transpose(-1, -2) @ qa) * scale,
        F_V=rows(smallP.transpose(-1, -2) @ da), F_Q=rows(smallS @ ka) * scale, F_K=rows(smallS.transpose(-1, -2) @ qa) * scale)


# ------------------------------------------------------------------------------------------------ bounds
def forward_bound(ref, dtype):
    b = 4 * U[dtype] * ref.A
    return b + ref.F if dtype == torch.float16 else b


def backward_bounds(ref, dtype):
    u, f16 = U[dtype], dtype == torch.float16
    dv = 3 * u * ref.A_V + (ref.F_V if f16 else 0)
    dq = 3 * u * ref.A_Q + CANCEL * ref.C_Q + (ref.F_Q if f16 else 0)
    dk = 3 * u * ref.A_K + CANCEL * ref.C_K + (ref.F_K if f16 else 0)
    return dict(dq=dq, dk=dk, dv=dv)


def _where(idx, shape, H):
    """flat index of a [B, n, H*D] tensor -> (b, row, head, channel)."""
    B, n, C = shape
    D = C // H
    b, r, c = idx // (n * C), (idx // C) % n, idx % C
    return b, r, c // D, c % D


def worst_ratio(got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def assert_within(name, got, ref, bound, H=1):
    """|got - ref| <= bound for every element; a failure names the worst element (b, row, head, channel), its ratio
    to the bound and how many elements exceed it."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), "%s: non-finite output" % name
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    bad = int((err > bound).sum())
    if bad:
        i = int(ratio.argmax())
        raise AssertionError("%s: %d of %d elements exceed the bound; worst at (b, row, head, channel) = %s: got %.6g, want %.6g, "
                             "|err| %.3e = %.2f x bound %.3e" % (name, bad, err.numel(), _where(i, ref.shape, H), float(got.flatten()[i]),
                                                                   float(ref.flatten()[i]), float(err.flatten()[i]), float(ratio.flatten()[i]),
                                                                   float(bound.flatten()[i])))
    return float(ratio.max())


def row_rms(got, ref, A, H, dtype, F=None):
    """[B, n, H]: RMS over a head's channels of |err| / (u A + F) -- F, the underflow term of the bound, for fp16 only."""
    B, n, C = ref.shape
    den = U[dtype] * A + (F if F is not None and dtype == torch.float16 else 0)
    r = (got.detach().double().cpu() - ref).abs() / den.clamp_min(1e-300)
    return r.reshape(B, n, H, C // H).pow(2).mean(-1).sqrt()


def assert_rows(name, got, ref, A, H, dtype, cap, F=None):
    r = row_rms(got, ref, A, H, dtype, F)
    bad = int((r > cap).sum())
    if bad:
        i = int(r.argmax())
        B, n, _ = r.shape
        raise AssertionError("%s: %d of %d rows exceed the row cap; worst at (b, row, head) = %s: RMS |err| / (u A + F) = %.3f > %.3f"
                             % (name, bad, r.numel(), (i // (n * H), (i // H) % n, i % H), float(r.flatten()[i]), cap))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ rounding model
def _round(x, dtype, flush):
    y = x.to(dtype).float()
    if flush and dtype == torch.float16:
        y = torch.where(x.abs() < FLUSH, torch.zeros_like(y), y)
    return y


def _group_any(g):
    """any() over groups of 32 consecutive rows (a wavefront's queries): [B, H, nq, 1] bool."""
    B, H, nq, _ = g.shape
    n32 = (nq + 31) // 32 * 32
    pad = torch.zeros(B, H, n32, dtype=torch.bool)
    pad[:, :, :nq] = g[..., 0]
    return pad.reshape(B, H, n32 // 32, 32).any(-1).repeat_interleave(32, -1)[:, :, :nq, None]


def emulate_forward(q, k, v, H, scale, bias=None, *, dtype, msum=False, splits=1, flush=False, tile=64, defer=8.0):
    """The forward kernels' rounding points in fp32.  msum: the denominator is the sum of the ROUNDED P.  splits > 1: the key
    tiles are cut into `splits` ranges of an even number of tiles, each leaves a normalised partial output rounded to `dtype`
    and an fp32 log-sum-exp; a weighted merge combines them.  Returns (out [B, nq, C] fp32 holding `dtype` values,
    lse [B, H, nq] fp32 -- of the unsplit walk only)."""
    f32 = torch.float32
    qh, kh, vh = heads(q, H, f32), heads(k, H, f32), heads(v, H, f32)
    s2 = qh @ kh.transpose(-1, -2) * scale
    if bias is not None:
        s2 = s2 + bias.float()
    s2 = s2 * LOG2E
    B, _, nq, nk = s2.shape

    def walk(a, b):
        m = torch.full((B, H, nq, 1), float("-inf"))
        l = torch.zeros(B, H, nq, 1)
        o = torch.zeros(B, H, nq, vh.shape[-1])
        for j in range(a, b, tile):
            sj = s2[..., j:min(j + tile, b)]
            m_new = torch.maximum(m, sj.amax(-1, keepdim=True))
            m_upd = torch.where(_group_any(m_new - m > defer), m_new, m) if defer > 0 else m_new
            alpha = torch.exp2(m - m_upd)
            l, o, m = l * alpha, o * alpha, m_upd
            p16 = _round(torch.exp2(sj - m), dtype, flush)
            l = l + (p16 if msum else torch.exp2(sj - m)).sum(-1, keepdim=True)
            o = o + p16 @ vh[:, :, j:min(j + tile, b)]
        return o / l, m + torch.log2(l)

    if splits <= 1:
        o, lse = walk(0, nk)
        return rows(_round(o, dtype, False)), lse.squeeze(-1)
    nkt = (nk + tile - 1) // tile
    per = (nkt + splits - 1) // splits
    per += per & 1
    parts = [walk(a, min(nk, a + per * tile)) for a in range(0, nk, per * tile)]
    lses = torch.stack([p[1] for p in parts])
    w = torch.exp2(lses - lses.amax(0))
    acc = sum(w[i] * _round(parts[i][0], dtype, False) for i in range(len(parts)))
    return rows(_round(acc / w.sum(0), dtype, False)), None


def emulate_backward(q, k, v, dout, lse, delta, H, scale, bias=None, *, dtype, flush=False):
    """The backward kernels' rounding points in fp32: P = exp2(s - lse) and dS = P (dp - delta) rounded to `dtype` before the
    second products, fp32 accumulation, outputs rounded once.  lse / delta fp32 [B, H, nq]."""
    f32 = torch.float32
    qh, kh, vh, doh = heads(q, H, f32), heads(k, H, f32), heads(v, H, f32), heads(dout, H, f32)
    s2 = qh @ kh.transpose(-1, -2) * scale
    if bias is not None:
        s2 = s2 + bias.float()
    p = torch.exp2(s2 * LOG2E - lse.float()[..., None])
    dp = doh @ vh.transpose(-1, -2)
    p16 = _round(p, dtype, flush)
    ds16 = _round(p * (dp - delta.float()[..., None]), dtype, flush)
    r = lambda x: rows(_round(x, dtype, False))
    return dict(dq=r(ds16 @ kh * scale), dk=r(ds16.transpose(-1, -2) @ qh * scale), dv=r(p16.transpose(-1, -2) @ doh))


# ------------------------------------------------------------------------------------------------ cases
def make_case(arm, B, H, D, nq, nk, **kw):
    c = dict(arm=arm, B=B, H=H, D=D, nq=nq, nk=nk, bias=False, scale=None, variant="normal", lse=False, vt_ld=None, fused=False,
             pp=0, S=1, msum=False, pad4=False, qs=1, qscale=1.0)
    c.update(kw)
    tags = [t for t in ("bias" if c["bias"] else "", c["variant"] if c["variant"] != "normal" else "", "lse" if c["lse"] else "",
                        "scale%g" % c["scale"] if c["scale"] is not None else "", "vtld%d" % c["vt_ld"] if c["vt_ld"] else "",
                        "fused" if c["fused"] else "", "pp%d" % c["pp"] if c["pp"] else "", "pad4" if c["pad4"] else "") if t]
    c["name"] = "-".join([arm, "x".join(str(x) for x in (B, H, D, nq, nk))] + tags)
    return SimpleNamespace(**c)


# (B, H, D, nq, nk) by dispatch arm of pf_attention; msum / S say which rounding model the arm follows
FWD_CASES = [
    # D = 64, no bias, short keys or lse requested: k_attention_lds<T, 64, false, false, 3>
    make_case("d64", 1, 2, 64, 33, 1), make_case("d64", 2, 2, 64, 200, 77), make_case("d64", 1, 2, 64, 130, 192),
    make_case("d64", 1, 8, 64, 160, 129), make_case("d64", 1, 2, 64, 64, 256, lse=True),
    # D = 64, MSUM (nk >= 256, no lse)
    make_case("d64msum", 1, 2, 64, 64, 256, msum=True), make_case("d64msum", 1, 2, 64, 96, 264, msum=True),
    make_case("d64msum", 2, 4, 64, 257, 320, msum=True),
    make_case("d64msum", 1, 1, 64, 32, 448, msum=True, variant="staircase"), make_case("d64msum", 1, 1, 64, 32, 448, msum=True, variant="spike"),
    # D = 32, no bias
    make_case("d32", 2, 4, 32, 128, 320), make_case("d32", 1, 2, 32, 96, 50), make_case("d32", 1, 3, 32, 33, 65),
    # D = 32, bias, unsplit
    make_case("d32bias", 2, 2, 32, 128, 256, bias=True, fused=True), make_case("d32bias", 1, 2, 32, 100, 132, bias=True),
    make_case("d32bias", 1, 2, 32, 100, 132, bias=True, scale=1.0, qscale=0.35), make_case("d32bias", 1, 2, 32, 100, 132, bias=True, scale=0.05),
    # D = 32, bias, split key range (S splits; run again unsplit)
    make_case("d32split", 1, 1, 32, 33, 1028, bias=True, S=2), make_case("d32split", 1, 2, 32, 64, 1536, bias=True, S=3),
    make_case("d32split", 2, 4, 32, 256, 4096, bias=True, S=8), make_case("d32split", 1, 2, 32, 64, 1536, bias=True, S=3, variant="spike"),
    # D = 64, bias: the register-pipelined form
    make_case("d64bias", 1, 2, 64, 100, 64, bias=True), make_case("d64bias", 1, 2, 64, 100, 128, bias=True), make_case("d64bias", 1, 2, 64, 100, 192, bias=True),
    make_case("d64bias", 1, 2, 64, 100, 260, bias=True), make_case("d64bias", 1, 2, 64, 100, 448, bias=True), make_case("d64bias", 1, 2, 64, 100, 192, bias=True, lse=True),
    # no-LDS fallback (vt_ld % 8 == 4)
    make_case("direct", 1, 2, 64, 33, 77, vt_ld=100), make_case("direct", 2, 2, 32, 100, 132, bias=True, vt_ld=164), make_case("direct", 1, 2, 64, 40, 96, vt_ld=100),
    # ping-pong kernels (denominator on the matrix pipe, as MSUM)
    make_case("pp", 1, 2, 64, 300, 136, pp=1, msum=True), make_case("pp", 1, 2, 64, 257, 256, pp=2, msum=True), make_case("pp", 1, 2, 64, 64, 384, pp=2, msum=True),
]

BWD_CASES = (
    [make_case("lds", B, 2, D, nq, nk, bias=bias) for D in (32, 64) for bias in (False, True) for (B, nq, nk) in ((2, 128, 320), (1, 64, 160))] +
    [make_case("ragged", 2, 2, 64, 16, 16), make_case("ragged", 2, 2, 64, 100, 128, bias=True), make_case("ragged", 2, 2, 32, 40, 72),
     make_case("whole", 1, 2, 64, 64, 96, pad4=True),
     make_case("qsplit", 1, 2, 32, 512, 64, qs=2), make_case("qsplit", 1, 1, 64, 544, 96, qs=2), make_case("qsplit", 1, 2, 64, 768, 160, bias=True, qs=3),
     # (appended: the seeds of the cases above follow their positions) a bias through the arms that ran without one
     make_case("ragged", 2, 2, 32, 40, 72, bias=True), make_case("whole", 1, 2, 32, 64, 96, pad4=True, bias=True),
     make_case("whole", 1, 2, 64, 96, 64, pad4=True, bias=True)])

STAIRS = (0, 12, 3, 10, 5, 9, 2)       # climb of the row maximum per 64-key tile, log2 units: above and below the 2^8 threshold
SPIKE_SPLIT = 20.0                     # spike key = 20 x a query row (D = 32: 163 log2 units above the rest -> the other splits' weights underflow)


def sparse_bias(nq, nk, gen, frac=0.2):
    """Bias that is non-zero in about `frac` of the 32 x 32 tiles, and the tile flags set from it."""
    nqt, nkt = (nq + 31) // 32, (nk + 31) // 32
    on = torch.rand(nqt, nkt, generator=gen) < frac
    on[-1, -1] = True                                       # (the ragged corner tile always carries a bias)
    full = torch.rand(nqt * 32, nkt * 32, generator=gen) * 2 * on.repeat_interleave(32, 0).repeat_interleave(32, 1)
    bias = full[:nq, :nk].contiguous()
    full.zero_()
    full[:nq, :nk] = bias
    flags = (full.reshape(nqt, 32, nkt, 32).abs().amax((1, 3)) > 0).to(torch.uint8)
    return bias, flags


def make_inputs(c, dtype, seed=0, backward=False):
    """Seeded inputs of a case, rounded to `dtype` (CPU): q [B, nq, C], k / v [B, nk, C], dout for a backward case, bias [nq, nk]
    fp32 + flags or None, and the softmax scale."""
    g = torch.Generator().manual_seed(1000 + seed)
    B, H, D, nq, nk = c.B, c.H, c.D, c.nq, c.nk
    C = H * D
    scale = c.scale if c.scale is not None else D ** -0.5
    q = torch.randn(B, nq, C, generator=g) * c.qscale
    k = torch.randn(B, nk, C, generator=g)
    v = torch.randn(B, nk, C, generator=g)
    if c.variant == "staircase":
        # keys aligned with the mean query direction, growing along the key index: the row maximum climbs tile after tile
        assert H == 1 and nk == 64 * len(STAIRS)
        d = torch.randn(D, generator=g)
        d = d / d.norm()
        q = 8.0 * d + 0.3 * torch.randn(B, nq, C, generator=g)
        level = torch.tensor(STAIRS, dtype=torch.float32).cumsum(0)
        t = torch.cat([level[i] - STAIRS[i] + STAIRS[i] * (torch.arange(64) + 1) / 64.0 for i in range(len(STAIRS))])     # log2 units
        k = d * (t / (8.0 * scale * LOG2E))[:, None] + 0.3 * torch.randn(B, nk, C, generator=g)
    q16 = q.to(dtype)
    if c.variant == "spike":
        row = min(5, nq - 1)
        if c.S > 1:                                         # in the middle split; every head
            k[0, nk // 2 - 68] = SPIKE_SPLIT * q16[0, row].float()
        else:
            k[0, nk * 2 // 3] = 3.0 * q16[0, row].float()
    bias = flags = None
    if c.bias:
        bias, flags = sparse_bias(nq, nk, g)
    out = SimpleNamespace(q=q16, k=k.to(dtype), v=v.to(dtype), bias=bias, flags=flags, scale=scale)
    if backward:
        out.dout = torch.randn(B, nq, C, generator=g).to(dtype)
    return out


def model_configs(c):
    """(msum, splits, tile, defer) of every launch the GPU test makes for a forward case."""
    if c.arm == "direct":
        return [(False, 1, 32, 0.0)]
    cfg = [(c.msum, c.S, 64, 8.0)]
    if c.S > 1:
        cfg.append((False, 1, 64, 8.0))                     # PF_ATTENTION_SPLIT=0
    return cfg


@functools.lru_cache(maxsize=None)
def fwd_ref(i, dtype):
    """(case, inputs, float64 reference) of FWD_CASES[i], computed once per process and shared by the test modules."""
    c = FWD_CASES[i]
    x = make_inputs(c, dtype, seed=i)
    return c, x, ref_forward(x.q, x.k, x.v, c.H, x.scale, x.bias)


@functools.lru_cache(maxsize=None)
def bwd_ref(i, dtype):
    c = BWD_CASES[i]
    x = make_inputs(c, dtype, seed=100 + i, backward=True)
    return c, x, ref_backward(x.q, x.k, x.v, x.dout, c.H, x.scale, x.bias)
