"""The attention kernels (forward arms of pf_attention, backward arms of pf_attention_bwd) against a float64 reference, per
ELEMENT and per ROW: |got - want| <= a derived multiple of u x the magnitude product (tests/attention_model.py), instead of one
rel-L2 over the tensor, which a wrong row, a bias flag read for the wrong tile or a split that drops a key tile passes.
Shapes are the smallest that reach each dispatch arm and each loop of it (steady trips, tails, ragged tiles, uneven splits);
operands sit in buffers with canaries around them.  Needs an MI355X: `-m gpu`.

Only the per-call switches are touched (PF_ATTENTION_PP, PF_ATTENTION_SPLIT); the arms behind once-per-process switches
are reached through their operand layouts (a V^T / transposed leading dimension that is 4 mod 8 takes the no-LDS kernels)."""
import pytest
import torch

import attention_model as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
KPAD = 64                # canary key rows after nk
OPAD = 8                 # canary columns on either side of an output


def ops():
    from panfusion_amd import ops as o
    return o


def report(arm, name, dtype, what, ratio, row):
    print("RATIO %-9s %-44s %-5s %-3s worst |err| / bound %.3f   worst row RMS / cap %.3f" % (arm, name, IDS[DTYPES.index(dtype)], what, ratio, row))


def padded_bias(bias, flags):
    """bias / flags as views of wider device buffers (bias_ld, flags_ld larger than needed; a read of the padding would dominate / flag)."""
    if bias is None:
        return None, None
    nq, nk = bias.shape
    big = torch.full((nq, nk + 12), 30.0, device=DEV)
    big[:, :nk] = bias.to(DEV)
    fbig = torch.ones(flags.shape[0], flags.shape[1] + 3, dtype=torch.uint8, device=DEV)
    fbig[:, :flags.shape[1]] = flags.to(DEV)
    return big[:, :nk], fbig[:, :flags.shape[1]]


def forward_operands(c, x, dtype):
    B, H, D, nq, nk, Cc = c.B, c.H, c.D, c.nq, c.nk, c.H * c.D
    if c.fused:                                               # one (q | k) buffer: q in columns [0, C) of its first nq rows, k in columns [C, 2C)
        wide = 2 * Cc
        qbuf = kbuf = torch.randn(B, max(nq, nk + KPAD), wide, device=DEV).to(dtype)
    else:
        wide = Cc
        qbuf = torch.randn(B, nq, wide, device=DEV).to(dtype)
        kbuf = torch.randn(B, nk + KPAD, wide, device=DEV).to(dtype)
    q, k = qbuf[:, :nq, :Cc], kbuf[:, :nk + KPAD, wide - Cc:]
    q.copy_(x.q.to(DEV))
    k[:, :nk] = x.k.to(DEV)
    k[:, nk:] = 8 * x.q.to(DEV)[:, :1]                        # rows past nk: 8 x a query row -- a read past nk would dominate the softmax
    vt_ld = c.vt_ld or (nk + 31) // 32 * 32
    vt = torch.full((B, Cc, vt_ld), float("nan"), dtype=dtype, device=DEV)     # padding must never be read as data
    vt[:, :, :nk] = x.v.to(DEV).transpose(1, 2)
    bias, flags = padded_bias(x.bias, x.flags)
    kw = dict(q_ld=wide, k_ld=wide, vt_ld=vt_ld, q_bs=q.stride(0), k_bs=k.stride(0), vt_bs=Cc * vt_ld, scale=x.scale, bias=bias, flags=flags)
    return q, k, vt, kw


def run_forward(c, q, k, vt, kw, dtype):
    """One launch into a column slice of a wider NaN buffer; returns (out, lse) and checks that the other columns stay NaN."""
    B, H, D, nq, nk, Cc = c.B, c.H, c.D, c.nq, c.nk, c.H * c.D
    o_ld = Cc + 2 * OPAD
    obuf = torch.full((B, nq, o_ld), float("nan"), dtype=dtype, device=DEV)
    out = obuf[:, :, OPAD:OPAD + Cc]
    lse = torch.full((B, H, nq), float("nan"), device=DEV) if c.lse else None
    ops().attention(q, k, vt, B, H, D, nq, nk, o_ld=o_ld, o_bs=nq * o_ld, out=out, lse=lse, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(obuf[:, :, :OPAD]).all() and torch.isnan(obuf[:, :, OPAD + Cc:]).all(), "%s: wrote outside its output columns" % c.name
    return out.float().cpu(), (lse.cpu() if c.lse else None)


def check_forward(c, ref, out, lse, dtype, what):
    name = "%s %s" % (c.name, what)
    ratio = M.worst_ratio(out, ref.O, M.forward_bound(ref, dtype))
    row = float(M.row_rms(out, ref.O, ref.A, c.H, dtype, ref.F).max()) / M.ROW_CAP_FWD
    report(c.arm, c.name, dtype, what, ratio, row)
    M.assert_within(name, out, ref.O, M.forward_bound(ref, dtype), c.H)
    M.assert_rows(name, out, ref.O, ref.A, c.H, dtype, M.ROW_CAP_FWD, ref.F)
    if c.lse:
        assert torch.isfinite(lse).all()
        err = (lse.double() - ref.lse).abs()
        assert float(err.max()) < 2e-4, "%s: lse off by %.3e at (b, head, row) flat index %d" % (name, float(err.max()), int(err.argmax()))


def assert_plan(c, q, k, vt, kw, dtype, S):
    """The library's plan of the launch run_forward is about to make: the kernel and the rounding arm (MSUM, S splits of the key range) the case claims --
    the bounds below follow that arm's rounding model."""
    lse = torch.empty(c.B, c.H, c.nq, device=DEV) if c.lse else None
    o_ld = c.H * c.D + 2 * OPAD
    g = ops().attention(q, k, vt, c.B, c.H, c.D, c.nq, c.nk, o_ld=o_ld, o_bs=c.nq * o_ld, lse=lse, want_plan=True, **kw)
    kernel = 0 if c.arm == "direct" else 1 + c.pp if c.pp else 1
    msum = c.msum and kernel == 1                             # (the ping-pong kernels always sum on the matrix pipe: no MSUM argument)
    assert (g.kernel, bool(g.msum), g.splits) == (kernel, msum, S), "%s plans to kernel %d, msum %d, %d splits" % (c.name, g.kernel, g.msum, g.splits)
    assert (g.workspace_bytes > 0) == (S > 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("i", range(len(M.FWD_CASES)), ids=[c.name for c in M.FWD_CASES])
def test_forward(i, dtype, monkeypatch):
    c, x, ref = M.fwd_ref(i, dtype)
    q, k, vt, kw = forward_operands(c, x, dtype)
    if c.pp:
        monkeypatch.setenv("PF_ATTENTION_PP", str(c.pp))
    assert_plan(c, q, k, vt, kw, dtype, c.S)
    out, lse = run_forward(c, q, k, vt, kw, dtype)
    check_forward(c, ref, out, lse, dtype, "S%d" % c.S if c.S > 1 else "")
    if c.S > 1:
        monkeypatch.setenv("PF_ATTENTION_SPLIT", "0")
        assert_plan(c, q, k, vt, kw, dtype, 1)
        out, lse = run_forward(c, q, k, vt, kw, dtype)
        check_forward(c, ref, out, lse, dtype, "S1")


# ------------------------------------------------------------------------------------------------ backward
def slot(B, n, Cc, dtype):
    """A [B, n, C] output as the middle columns of a wider zero-filled buffer."""
    buf = torch.zeros(B, n, Cc + 2 * OPAD, dtype=dtype, device=DEV)
    return buf, buf[:, :, OPAD:OPAD + Cc]


def transposed(x, pad):
    """[B, n, C] -> [B, C, n] with the rows padded by `pad` NaN tokens (the leading dimension is n + pad)."""
    B, n, Cc = x.shape
    buf = torch.full((B, Cc, n + pad), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, :, :n] = x.transpose(1, 2)
    return buf[:, :, :n]


def backward_operands(c, x, ref, dtype):
    """Device operands of a backward case and the keywords of ops.attention_bwd: contiguous q / k / v / dout, their transposes (rows
    padded by 4 NaN tokens under pad4), lse / delta from the reference (the bound judges the backward kernels alone), outputs in slots."""
    B, H, D, nq, nk, Cc = c.B, c.H, c.D, c.nq, c.nk, c.H * c.D
    q, k, v, dout = (t.to(DEV).contiguous() for t in (x.q, x.k, x.v, x.dout))
    pad = 4 if c.pad4 else 0
    qt, kt, dot = transposed(q, pad), transposed(k, pad), transposed(dout, pad)
    lse, delta = ref.lse.float().to(DEV).contiguous(), ref.delta.float().to(DEV).contiguous()
    bias, flags = padded_bias(x.bias, x.flags)
    slots = slot(B, nq, Cc, dtype), slot(B, nk, Cc, dtype), slot(B, nk, Cc, dtype)
    w = Cc + 2 * OPAD
    args = (q, k, v, dout, qt, kt, dot, lse, delta, slots[0][1], slots[1][1], slots[2][1], B, H, D, nq, nk)
    kw = dict(q_ld=Cc, k_ld=Cc, v_ld=Cc, do_ld=Cc, dq_ld=w, dk_ld=w, dv_ld=w, q_bs=nq * Cc, k_bs=nk * Cc, v_bs=nk * Cc, do_bs=nq * Cc,
              dq_bs=nq * w, dk_bs=nk * w, dv_bs=nk * w, scale=x.scale, bias=bias, flags=flags)
    return args, kw, slots


def run_backward(c, args, kw, slots):
    for buf, _ in slots:
        buf.zero_()
    ops().attention_bwd(*args, **kw)
    torch.cuda.synchronize()
    for buf, _ in slots:                                   # the slots the call does not own stay zero
        Cc = c.H * c.D
        assert not buf[:, :, :OPAD].any() and not buf[:, :, OPAD + Cc:].any(), "%s: wrote outside its output columns" % c.name
    return dict(dq=slots[0][1].clone(), dk=slots[1][1].clone(), dv=slots[2][1].clone())


BWD_KERNEL = {"whole": 0, "ragged": 1, "lds": 2, "qsplit": 2}


def assert_bwd_plan(c, args, kw):
    """The library's plan of the launch run_backward is about to make: the kernel pair and the query split the case claims -- the bounds
    below belong to that arm."""
    g = ops().attention_bwd(*args, want_plan=True, **kw)
    assert (g.kernel, g.qsplit) == (BWD_KERNEL[c.arm], c.qs), "%s plans to kernel %d, qsplit %d" % (c.name, g.kernel, g.qsplit)
    assert (g.workspace_bytes > 0) == (c.qs > 1) == (g.reduce_grid_x > 0)


BWD = (("dq", "dQ", "A_Q", "F_Q"), ("dk", "dK", "A_K", "F_K"), ("dv", "dV", "A_V", "F_V"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("i", range(len(M.BWD_CASES)), ids=[c.name for c in M.BWD_CASES])
def test_backward(i, dtype):
    c, x, ref = M.bwd_ref(i, dtype)
    args, kw, slots = backward_operands(c, x, ref, dtype)
    assert_bwd_plan(c, args, kw)
    got = run_backward(c, args, kw, slots)
    if c.qs > 1:
        again = run_backward(c, args, kw, slots)           # partial sums are added in a fixed order
        assert torch.equal(again["dk"], got["dk"]) and torch.equal(again["dv"], got["dv"])
    bounds = M.backward_bounds(ref, dtype)
    fails = []
    for n, R, A, F in BWD:
        want, mag, und = getattr(ref, R), getattr(ref, A), getattr(ref, F)
        out = got[n].float().cpu()
        report(c.arm, c.name, dtype, n, M.worst_ratio(out, want, bounds[n]), float(M.row_rms(out, want, mag, c.H, dtype, und).max()) / M.ROW_CAP_BWD)
        try:
            M.assert_within("%s %s" % (c.name, n), out, want, bounds[n], c.H)
            M.assert_rows("%s %s" % (c.name, n), out, want, mag, c.H, dtype, M.ROW_CAP_BWD, und)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
