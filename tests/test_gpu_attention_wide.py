"""pf_attention_wide (flash attention at head widths 128 / 256 / 512) on the GPU: every case of attention_wide_cases.WIDE_CASES
against the float64 reference per element and per row (tests/attention_model.py) and against the materialised three-launch form;
strided operands with canaries; determinism; the 1024 x 2176 panorama's mid-block size (34 816 tokens, D = 512) once, with 256
rows held to the float64 bound and the whole output to the query-chunked materialised form.  Needs an MI355X: `-m gpu`."""
import pytest
import torch

import attention_model as M
import attention_wide_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
KPAD = 64                # canary key rows after nk
OPAD = 8                 # canary columns on either side of an output


def ops():
    from panfusion_amd import ops as o
    return o


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def operands(c, x, dtype, pad=0, vt_ld=None, bs_extra=0):
    """q, k, V^T of a case on the GPU inside larger buffers: `pad` extra columns per q / k row, KPAD canary key rows (8 x a query
    row: a read past nk would dominate the softmax), NaN in the padding of V^T, `bs_extra` unused rows between the batches."""
    B, nq, nk, Cc = c.B, c.nq, c.nk, c.H * c.D
    wide = Cc + pad
    qbuf = torch.randn(B, nq + bs_extra, wide, device=DEV).to(dtype)
    kbuf = torch.randn(B, nk + KPAD + bs_extra, wide, device=DEV).to(dtype)
    q, k = qbuf[:, :nq, :Cc], kbuf[:, :nk + KPAD, :Cc]
    q.copy_(x.q.to(DEV))
    k[:, :nk] = x.k.to(DEV)
    k[:, nk:] = 8 * x.q.to(DEV)[:, :1]
    vt_ld = vt_ld or (nk + 31) // 32 * 32
    vbuf = torch.full((B, Cc + bs_extra, vt_ld), float("nan"), dtype=dtype, device=DEV)
    vt = vbuf[:, :Cc]
    vt[:, :, :nk] = x.v.to(DEV).transpose(1, 2)
    kw = dict(q_ld=wide, k_ld=wide, vt_ld=vt_ld, q_bs=qbuf.stride(0), k_bs=kbuf.stride(0), vt_bs=vbuf.stride(0), scale=x.scale)
    return q, k, vt, kw


def run(c, q, k, vt, kw, dtype, bs_extra=0):
    """One launch into a column slice of a wider NaN buffer; the columns (and the rows between batches) it does not own stay NaN."""
    B, nq, nk, Cc = c.B, c.nq, c.nk, c.H * c.D
    o_ld = Cc + 2 * OPAD
    obuf = torch.full((B, nq + bs_extra, o_ld), float("nan"), dtype=dtype, device=DEV)
    out = obuf[:, :nq, OPAD:OPAD + Cc]
    ops().attention_wide(q, k, vt, B, c.H, c.D, nq, nk, o_ld=o_ld, o_bs=obuf.stride(0), out=out, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(obuf[:, :, :OPAD]).all() and torch.isnan(obuf[:, :, OPAD + Cc:]).all(), "%s: wrote outside its output columns" % c.name
    assert torch.isnan(obuf[:, nq:]).all(), "%s: wrote outside its output rows" % c.name
    return out.float().cpu()


def check(c, ref, out, dtype, what=""):
    name = "%s %s" % (c.name, what)
    bound = M.forward_bound(ref, dtype)
    ratio = M.worst_ratio(out, ref.O, bound)
    row = float(M.row_rms(out, ref.O, ref.A, c.H, dtype, ref.F).max())
    print("RATIO wide %-36s %-4s %-8s worst |err| / bound %.3f   worst row RMS %.3f (cap %.2f)" % (c.name, IDS[DTYPES.index(dtype)], what, ratio, row, W.ROW_CAP_WIDE))
    M.assert_within(name, out, ref.O, bound, c.H)
    M.assert_rows(name, out, ref.O, ref.A, c.H, dtype, W.ROW_CAP_WIDE, ref.F)


def materialised(x, c, dtype):
    """The three-launch form (scores GEMM, row softmax, P V GEMM) per batch and head, on operands padded to the GEMM's multiples of 64."""
    o = ops()
    B, H, D, nq, nk = c.B, c.H, c.D, c.nq, c.nk
    nqp, nkp = (nq + 63) // 64 * 64, (nk + 63) // 64 * 64
    out = torch.empty(B, nq, H * D)
    for b in range(B):
        for h in range(H):
            cols = slice(h * D, (h + 1) * D)
            q = torch.zeros(nqp, D, dtype=dtype, device=DEV)
            k = torch.zeros(nkp, D, dtype=dtype, device=DEV)
            vt = torch.zeros(D, nkp, dtype=dtype, device=DEV)
            q[:nq], k[:nk], vt[:, :nk] = x.q[b, :, cols].to(DEV), x.k[b, :, cols].to(DEV), x.v[b, :, cols].to(DEV).t()
            s = o.conv_gemm(q, k, nkp, w_in=nqp, out_dtype=torch.float32)
            p = torch.zeros(nqp, nkp, dtype=dtype, device=DEV)
            o.softmax_rows(s[:, :nk], x.scale, dtype, out=p[:, :nk])
            out[b, :, cols] = o.conv_gemm(p, vt, D, w_in=nqp)[:nq].float().cpu()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("i", range(len(W.WIDE_CASES)), ids=[c.name for c in W.WIDE_CASES])
def test_forward(i, dtype):
    c, x, ref = W.wide_ref(i, dtype)
    q, k, vt, kw = operands(c, x, dtype)
    out = run(c, q, k, vt, kw, dtype)
    check(c, ref, out, dtype)
    old = rel_l2(out, materialised(x, c, dtype))
    print("RATIO wide %-36s %-4s rel-L2 vs the materialised form %.3e (tolerance %.1e)" % (c.name, IDS[DTYPES.index(dtype)], old, M.OLD_TOL[dtype]))
    assert old <= M.OLD_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("vt_ld", [104, 100], ids=["vtld104", "vtld100"])
def test_strided_operands(vt_ld, dtype):
    """q_ld, k_ld, o_ld larger than H * D, vt_ld larger than nk rounded up (a multiple of 8, and 4 mod 8: the 8-byte V^T loads), a batch
    stride larger than the tensor; the output's padding columns and the rows between the batches keep their sentinel."""
    i = 1                                                      # (2, 1, 512, 100, 77)
    c, x, ref = W.wide_ref(i, dtype)
    q, k, vt, kw = operands(c, x, dtype, pad=24, vt_ld=vt_ld, bs_extra=3)
    out = run(c, q, k, vt, kw, dtype, bs_extra=3)
    check(c, ref, out, dtype, "vt_ld%d" % vt_ld)


def test_two_heads_strided():
    """H = 2 with padded rows: head h sits at column h * D of q, k and out, at row h * D of V^T."""
    i, dtype = 6, torch.float16                                # (1, 2, 256, 70, 200)
    c, x, ref = W.wide_ref(i, dtype)
    q, k, vt, kw = operands(c, x, dtype, pad=8, vt_ld=232)
    check(c, ref, run(c, q, k, vt, kw, dtype), dtype, "pad8")


@pytest.mark.parametrize("i", [1, 5], ids=[W.WIDE_CASES[1].name, W.WIDE_CASES[5].name])
def test_deterministic(i):
    dtype = torch.float16
    c, x, _ = W.wide_ref(i, dtype)
    q, k, vt, kw = operands(c, x, dtype)
    a, b = run(c, q, k, vt, kw, dtype), run(c, q, k, vt, kw, dtype)
    assert torch.equal(a, b)


def test_full_size():
    """B = 1, H = 1, D = 512, nq = nk = 34 816 (the padded 1024 x 2176 panorama at the VAE's mid-block), fp16, run once: 256 query rows --
    the first 64, the last 64, 128 seeded random ones -- against float64 (bound and row cap), the whole output against the
    query-chunked materialised form on the GPU."""
    from panfusion_amd import vae
    dtype, N, D = torch.float16, 34816, 512
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(1, N, D, generator=g).to(dtype) for _ in range(3))
    qd, kd = q.to(DEV), k.to(DEV)
    vt = v.to(DEV).transpose(1, 2).contiguous()
    out = ops().attention_wide(qd, kd, vt, 1, 1, D, N, N, q_ld=D, k_ld=D, vt_ld=N, q_bs=N * D, k_bs=N * D, vt_bs=D * N)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    idx = torch.cat([torch.arange(64), torch.arange(N - 64, N), 64 + torch.randperm(N - 128, generator=g)[:128]])
    ref = M.ref_forward(q[:, idx], k, v, 1, D ** -0.5)
    c = M.make_case("wide-full", 1, 1, D, len(idx), N)
    check(c, ref, out[:, idx.to(DEV)].float().cpu(), dtype, "256 rows")
    plan = vae.attention_plan(1, N, D, dtype, "materialised")
    assert plan.rows < N and plan.rows % 64 == 0
    old = torch.empty(N, D, dtype=dtype, device=DEV)
    for rows, o in vae.materialised_attention(qd.view(N, D), kd.view(N, D), vt, 1, N, D, dtype, plan):
        old[rows] = o
    r = rel_l2(out.view(N, D).float(), old.float())
    print("RATIO wide full size: rel-L2 vs the query-chunked materialised form %.3e (tolerance %.1e)" % (r, M.OLD_TOL[dtype]))
    assert r <= M.OLD_TOL[dtype]
