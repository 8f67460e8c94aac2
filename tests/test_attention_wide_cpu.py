"""CPU side of the wide-head flash attention (pf_attention_wide) and of the VAE's choice of attention form: the rounding model's
maxima at the kernel's configuration (they set ROW_CAP_WIDE), argument rejection before any launch (the library loads without a
GPU, as in test_abi.py), and the pure planner vae.attention_plan."""
import ctypes as C

import pytest
import torch

import attention_model as M
import attention_wide_cases as W
from panfusion_amd import _lib

DTYPES = [torch.bfloat16, torch.float16]


def test_cases_are_the_listed_ones():
    got = [(c.B, c.H, c.D, c.nq, c.nk, c.variant) for c in W.WIDE_CASES]
    assert got == [(1, 1, 512, 33, 1, "normal"), (2, 1, 512, 100, 77, "normal"), (1, 1, 512, 130, 192, "normal"),
                   (1, 1, 512, 64, 448, "staircase"), (1, 1, 512, 64, 448, "spike"), (2, 1, 512, 96, 1100, "normal"),
                   (1, 2, 256, 70, 200, "normal"), (1, 1, 128, 70, 200, "normal")]


def test_model_maxima():
    """The rounding model at the kernel's (msum, tile, defer), both types, fp16 subnormals of P kept and flushed: every element inside
    the float64 bound, the underflow term F small against u A, and the recorded maxima -- which fix ROW_CAP_WIDE -- still hold."""
    elem = row = fmed = 0.0
    for i, c in enumerate(W.WIDE_CASES):
        for dtype in DTYPES:
            _, x, ref = W.wide_ref(i, dtype)
            for flush in (False, True):
                out, _ = M.emulate_forward(x.q, x.k, x.v, c.H, x.scale, dtype=dtype, flush=flush, **W.KERNEL_MODEL)
                elem = max(elem, M.worst_ratio(out, ref.O, M.forward_bound(ref, dtype)))
                row = max(row, float(M.row_rms(out, ref.O, ref.A, c.H, dtype, ref.F).max()))
            if dtype == torch.float16:
                fmed = max(fmed, float((ref.F / (M.U[dtype] * ref.A)).median()))
    print("model maxima, wide cases: element ratio %.3f, row RMS %.3f, median F / (u A) %.3f" % (elem, row, fmed))
    assert elem <= 1.0 and fmed < 0.1
    assert elem <= W.MODEL_MAX_WIDE["ELEM"] * 1.02 and row <= W.MODEL_MAX_WIDE["ROW"] * 1.02 and fmed <= W.MODEL_MAX_WIDE["F_MEDIAN"] * 1.02
    # the cap is twice the model's largest row RMS, rounded up to two decimals -- never taken from the kernel
    assert W.ROW_CAP_WIDE == pytest.approx(-(-2 * W.MODEL_MAX_WIDE["ROW"] * 100 // 1) / 100)
    assert 2 * row <= W.ROW_CAP_WIDE


def _desc(**kw):
    """A structurally valid D = 512 problem on fake (never dereferenced) device addresses; kw overrides fields."""
    a = _lib.AttnDesc()
    a.q, a.k, a.vt, a.out = 0x10000, 0x20000, 0x30000, 0x40000
    a.dtype, a.B, a.H, a.D, a.nq, a.nk = _lib.PF_F16, 2, 1, 512, 100, 77
    a.q_ld = a.k_ld = a.o_ld = 512
    a.vt_ld = 96
    a.q_bs, a.k_bs, a.vt_bs, a.o_bs = 100 * 512, 77 * 512, 512 * 96, 100 * 512
    a.scale = 512 ** -0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD = [
    (dict(D=48), b"head dim"), (dict(D=64), b"head dim"), (dict(D=32), b"head dim"),
    (dict(bias=0x50000), b"bias"), (dict(flags=0x50000), b"flags"), (dict(bias=0x50000, flags=0x60000, bias_ld=80, flags_ld=4), b"bias"),
    (dict(lse=0x50000), b"lse"), (dict(workspace=0x50000, workspace_bytes=1 << 20), b"workspace"),
    (dict(vt_ld=64), b"vt_ld"), (dict(vt_ld=92), b"vt_ld"),
    (dict(q=0x10008), b"16-byte aligned"), (dict(vt=0x30004), b"16-byte aligned"), (dict(out=0x40002), b"16-byte aligned"),
    (dict(q_ld=516), b"leading dimensions"), (dict(k_ld=514), b"leading dimensions"), (dict(o_ld=518), b"leading dimensions"), (dict(vt_ld=98), b"leading dimensions"),
    (dict(q_ld=256), b"cover"), (dict(o_ld=504), b"cover"),
    (dict(q_bs=100 * 512 + 4), b"batch strides"), (dict(vt_bs=512 * 96 + 2), b"batch strides"), (dict(o_bs=100 * 512 + 2), b"batch strides"),
    (dict(q=0), b"null pointer"), (dict(out=0), b"null pointer"),
    (dict(nk=0), b"bad sizes"), (dict(B=0), b"bad sizes"),
    (dict(dtype=_lib.PF_F32), b"dtype"),
    (dict(nk=(1 << 21), vt_ld=(1 << 21), k_bs=(1 << 30), vt_bs=(1 << 30)), b"per-batch operand too large"),
    (dict(D=128, nq=(1 << 30), B=128, q_ld=128, k_ld=128, o_ld=128), b"grid"),
]


@pytest.mark.parametrize("kw,needle", BAD, ids=["-".join("%s=%s" % (k, hex(v) if v > 4096 else v) for k, v in kw.items()) for kw, _ in BAD])
def test_rejects_bad_arguments_before_any_launch(kw, needle):
    lib = _lib.lib()
    assert lib.pf_attention_wide(C.byref(_desc(**kw)), None) == 1, kw            # PF_ERR_ARG
    msg = lib.pf_last_error_string()
    assert b"pf_attention_wide" in msg and needle in msg, (kw, msg)


def test_null_descriptor():
    lib = _lib.lib()
    assert lib.pf_attention_wide(None, None) == 1 and b"pf_attention_wide" in lib.pf_last_error_string()


# ------------------------------------------------------------------------------------------------ vae.attention_plan
def test_attention_plan_keeps_the_sizes_that_ran_before():
    from panfusion_amd import vae
    for (n, N), per in (((20, 4096), 8), ((1, 5120), 1), ((3, 256), 3), ((1, 23104), 1), ((7, 4096), 7), ((40, 1024), 8)):
        for mode in ("auto", "materialised"):
            for dtype in DTYPES:
                p = vae.attention_plan(n, N, 512, dtype, mode)
                assert (p.form, p.per, p.rows) == ("materialised", per, N), (n, N, mode, vars(p))
        # what _attention computed before the flash kernel existed
        old = min(max(1, min(n, (1 << 31) // (N * N * 4))) if N * N * 4 < (1 << 31) else 1, 8)
        assert old == per


def test_attention_plan_beyond_the_limit():
    from panfusion_amd import vae
    N = 34816
    # measured (profiles/wide_attention_ab.txt): at this size the query-chunked materialised form is the faster one, so "auto" takes it;
    # the flash kernel is chosen by name
    p = vae.attention_plan(1, N, 512, torch.float16, "auto")
    assert (p.form, p.per, p.rows) == ("materialised", 1, 11648)
    p = vae.attention_plan(1, N, 512, torch.float16, "flash")
    assert (p.form, p.per, p.rows) == ("flash", 1, N)
    assert vae.attention_plan(1, N, 128, torch.bfloat16, "flash").form == "flash"
    for Cc, dtype in ((384, torch.float16), (512, torch.float32)):               # a width / type the kernel does not serve
        p = vae.attention_plan(1, N, Cc, dtype, "auto")
        assert p.form == "materialised" and p.per == 1 and p.rows < N
        with pytest.raises(ValueError):
            vae.attention_plan(1, N, Cc, dtype, "flash")
    for n, Ntok, limit in ((1, N, (1 << 31) - 1), (2, N, (1 << 31) - 1), (1, 46400, (1 << 31) - 1), (1, 2560, 4 << 20), (3, 2560, 1 << 20), (1, 4096, 3 << 20)):
        p = vae.attention_plan(n, Ntok, 512, torch.float16, "materialised", max_operand_bytes=limit)
        assert p.form == "materialised" and p.per == 1 and p.rows % 64 == 0 and 0 < p.rows < Ntok
        assert p.rows * Ntok * 4 <= limit and p.rows * Ntok * 2 <= limit         # fp32 scores and 16-bit P of a chunk
        chunks = -(-Ntok // p.rows)
        assert (chunks - 1) * (limit // (Ntok * 4) // 64 * 64) < Ntok            # no fewer chunks would do
    assert vae.attention_plan(20, 4096, 512, torch.float16, "flash").form == "flash"     # flash on request at a size that fits


def test_attention_plan_rejects_bad_modes():
    from panfusion_amd import vae
    for mode in ("Flash", "", None, "tiled", 1):
        with pytest.raises(ValueError):
            vae.attention_plan(1, 4096, 512, torch.float16, mode)
        with pytest.raises(ValueError):
            vae.VAEDecoder(None, attention=mode)
        with pytest.raises(ValueError):
            vae.VAEEncoder(None, attention=mode)
    assert vae.VAEDecoder(None).attention == "auto" and vae.VAEEncoder(None, attention="flash").attention == "flash"


# ------------------------------------------------------------------------------------------------ engine.row_ranges
def test_row_ranges():
    """The pixel-row planner of the host-side splits: the ranges cover the rows once and in order, each fits the limit, no fewer
    ranges would do, their sizes differ by at most one row; the 1024 x 2176 x 256 fp32 shortcut operand gives 2."""
    from panfusion_amd import engine, vae
    assert vae.row_ranges is engine.row_ranges
    G = (1 << 31) - 1
    assert engine.row_ranges(1024 * 2176, 256 * 4) == [(0, 1114112), (1114112, 2228224)]
    assert engine.row_ranges(512 * 1088, 256 * 4) == [(0, 512 * 1088)]                     # a size that ran before: one range, the launch of before
    for rows, row_bytes, limit in ((1024 * 2176, 1024, G), (1024 * 2176, 2048, G), (163840, 1024, 50 << 20), (40960, 2048, 50 << 20),
                                   (7, 8, 8), (7, 8, 23), (7, 8, 24), (1000, 12, 4000), (1, 512, 512), (99991, 640, 1 << 20)):
        r = engine.row_ranges(rows, row_bytes, limit)
        assert r[0][0] == 0 and r[-1][1] == rows and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(b > a for a, b in r)
        sizes = [b - a for a, b in r]
        assert max(sizes) * row_bytes <= limit and max(sizes) - min(sizes) <= 1
        assert (len(r) - 1) * (limit // row_bytes) < rows                                   # the fewest ranges
    for bad in ((0, 8, 64), (8, 0, 64), (8, 128, 64)):
        with pytest.raises(ValueError):
            engine.row_ranges(*bad)
