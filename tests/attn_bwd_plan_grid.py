"""The fixed grid of pf_attention_bwd problems behind tests/golden/attn_bwd_plans.npz (tools/make_golden_attn_bwd_plans.py writes it,
tests/test_attn_bwd_plans.py reruns it): descriptors on fake, never dereferenced pointers, pf_attention_bwd_workspace_size and the whole
pf_attn_bwd_plan of each, under every setting of the two PF_ATTN_BWD_* knobs.  The planner reads both once per process, so every
non-default setting gets a child process (this file run as a script).  Host arithmetic only: no GPU is opened."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import attention_model as M  # noqa: E402
from panfusion_amd import _lib  # noqa: E402

KNOBS = ("PF_ATTN_BWD_IMPL", "PF_ATTN_BWD_QSPLIT")
ENVS = ({}, {"PF_ATTN_BWD_IMPL": "direct"}, {"PF_ATTN_BWD_QSPLIT": "0"})
PLAN_FIELDS = tuple(f for f, _ in _lib.AttnBwdPlan._fields_)
COLUMNS = ("workspace_size",) + PLAN_FIELDS
OPAD = 8                 # canary columns on either side of an output in tests/test_gpu_attention_bounds.py


def prob(tag, B, H, D, nq, nk, bias=False, wide=1, kwide=None, o_ld=None, qt_ld=None, kt_ld=None, dot_ld=None, qt_bs=None, kt_bs=None,
         dot_bs=None):
    """wide / kwide: q and k | v sit in buffers of wide / kwide x H * D columns (fused projections; kwide defaults to wide); so do the
    outputs (unless o_ld gives their leading dimension) and, as row slices of the buffers' transposes, Q^T and K^T.  qt_ld / kt_ld /
    dot_ld: the transposed leading dimensions (default: the token count); qt_bs / kt_bs / dot_bs: their batch strides (default: the rows
    of the transposed buffer x the leading dimension)."""
    return dict(tag=tag, B=B, H=H, D=D, nq=nq, nk=nk, bias=bias, wide=wide, kwide=kwide or wide, o_ld=o_ld, qt_ld=qt_ld, kt_ld=kt_ld,
                dot_ld=dot_ld, qt_bs=qt_bs, kt_bs=kt_bs, dot_bs=dot_bs)


def bwd_case_problem(c):
    """BWD_CASES entry -> the descriptor test_gpu_attention_bounds.py launches: contiguous operands, transposes whose rows are padded by
    4 tokens under pad4, outputs inside wider buffers."""
    pad = 4 if c.pad4 else 0
    return prob("bwd:" + c.name, c.B, c.H, c.D, c.nq, c.nk, bias=c.bias, o_ld=c.H * c.D + 2 * OPAD, qt_ld=c.nq + pad, kt_ld=c.nk + pad,
                dot_ld=c.nq + pad)


# The backward launches of bench.py's training leg (one sample: 20 views of 32 x 32 latents, the 64 x 128 panorama).  Self-attention of
# every level, views then panorama, on the fused (q | k | v) projection: (B, H, nq = nk) at D = 64
TRAIN_SELF = ((20, 5, 1024), (20, 10, 256), (20, 20, 64), (20, 20, 16), (1, 5, 8192), (1, 10, 2048), (1, 20, 512), (1, 20, 128))
TEXT_PAD = 128           # the text cross-attention of the same levels: 77 keys padded to 128 under a bias, k | v fused
# the two EPA directions (D = 32, bias; panorama tokens x view tokens, then the reverse): (H, panorama tokens, view tokens)
TRAIN_EPA = ((10, 2048, 5120), (20, 2048, 5120), (20, 512, 1280), (40, 512, 1280), (40, 128, 320))


def problems():
    """Every problem of the grid (the order is part of the fixture)."""
    out = [bwd_case_problem(c) for c in M.BWD_CASES]
    out += [prob("train_self", B, H, 64, n, n, wide=3) for B, H, n in TRAIN_SELF]
    out += [prob("train_text", B, H, 64, n, TEXT_PAD, bias=True, kwide=2) for B, H, n in TRAIN_SELF]
    out += [prob("train_epa", 1, H, 32, e, v, bias=True, wide=3) for H, e, v in TRAIN_EPA]
    out += [prob("train_epa", 1, H, 32, v, e, bias=True, wide=3) for H, e, v in TRAIN_EPA]
    # base = ceil(nk / 128) * H * B against 384: 383 splits, 384 does not
    out += [prob("base_edge", 1, 383, 32, 512, 128), prob("base_edge", 1, 384, 32, 512, 128), prob("base_edge", 383, 1, 64, 512, 96),
            prob("base_edge", 2, 192, 64, 512, 64), prob("base_edge", 1, 128, 32, 512, 384), prob("base_edge", 1, 127, 32, 512, 384)]
    # (nq / 32) / 8 = 0, 1, 1, 2 ...
    out += [prob("nq_edge", 1, 2, 64, nq, 128) for nq in (224, 256, 480, 512)]
    # ... binding (8192 queries = 32, base 2) against ceil(512 / base) binding (base 200 -> 3, 100 -> 6, 300 -> 2); both 512 at base 1
    out += [prob("bind", 1, 2, 64, 8192, 128), prob("bind", 1, 200, 32, 8192, 128), prob("bind", 2, 50, 32, 8192, 96),
            prob("bind", 1, 1, 64, 1 << 17, 128), prob("bind", 1, 300, 32, 8192, 128)]
    # one transposed operand each whose rows are 4 mod 8 elements, one batch stride each that is 4 mod 8: the LDS kernels need both
    out += [prob("align", 1, 2, 64, 512, 128, qt_ld=516), prob("align", 1, 2, 64, 512, 128, kt_ld=132), prob("align", 1, 2, 64, 512, 128, dot_ld=516),
            prob("align", 2, 2, 32, 512, 128, qt_bs=64 * 512 + 4), prob("align", 2, 2, 32, 512, 128, kt_bs=64 * 128 + 4),
            prob("align", 2, 2, 32, 512, 128, dot_bs=64 * 512 + 4), prob("align", 2, 2, 32, 512, 128, qt_bs=64 * 512 + 8)]
    # ragged on one side only
    out += [prob("ragged", 1, 2, 64, 500, 128), prob("ragged", 1, 2, 64, 512, 100, bias=True), prob("ragged", 2, 2, 32, 16, 64),
            prob("ragged", 1, 2, 32, 520, 72)]
    return out


def descriptor(tag, B, H, D, nq, nk, bias, wide, kwide, o_ld, qt_ld, kt_ld, dot_ld, qt_bs, kt_bs, dot_bs):
    Cc = H * D
    d = _lib.AttnBwdDesc()
    for i, f in enumerate(("q", "k", "v", "dout", "qt", "kt", "dot", "dq", "dk", "dv", "lse", "delta")):
        setattr(d, f, 0x100000 * (i + 1))
    d.dtype, d.B, d.H, d.D, d.nq, d.nk = _lib.PF_BF16, B, H, D, nq, nk
    d.q_ld, d.k_ld, d.v_ld, d.do_ld = wide * Cc, kwide * Cc, kwide * Cc, Cc
    d.dq_ld, d.dk_ld, d.dv_ld = o_ld or wide * Cc, o_ld or kwide * Cc, o_ld or kwide * Cc
    d.qt_ld, d.kt_ld, d.dot_ld = qt_ld or nq, kt_ld or nk, dot_ld or nq
    d.q_bs, d.k_bs, d.v_bs, d.do_bs = nq * d.q_ld, nk * d.k_ld, nk * d.v_ld, nq * Cc
    d.dq_bs, d.dk_bs, d.dv_bs = nq * d.dq_ld, nk * d.dk_ld, nk * d.dv_ld
    d.qt_bs, d.kt_bs, d.dot_bs = qt_bs or wide * Cc * d.qt_ld, kt_bs or kwide * Cc * d.kt_ld, dot_bs or Cc * d.dot_ld
    d.scale = D ** -0.5
    if bias:
        d.bias, d.bias_ld, d.flags, d.flags_ld = 0x5000000, nk, 0x6000000, (nk + 31) // 32
    return d


def load(path=None):
    """The attention-backward queries of the library at `path` (default: the one panfusion_amd uses), bound directly: a library from
    before pf_attention_bwd_plan existed loads too and has has_plan False."""
    import torch  # noqa: F401  (the library resolves the HIP runtime torch ships, as panfusion_amd._lib does)
    lib = C.CDLL(path or _lib.LIB_PATH)
    lib.pf_attention_bwd_workspace_size.restype, lib.pf_attention_bwd_workspace_size.argtypes = _lib.SIGNATURES["pf_attention_bwd_workspace_size"]
    lib.has_plan = hasattr(lib, "pf_attention_bwd_plan")
    if lib.has_plan:
        lib.pf_attention_bwd_plan.restype, lib.pf_attention_bwd_plan.argtypes = _lib.SIGNATURES["pf_attention_bwd_plan"]
    return lib


def plan(lib, d):
    g = _lib.AttnBwdPlan()
    assert lib.pf_attention_bwd_plan(C.byref(d), C.byref(g)) == 0
    return g


def row(lib, d):
    """One fixture row: COLUMNS of descriptor d (the plan columns -1 for a library without pf_attention_bwd_plan)."""
    ws = lib.pf_attention_bwd_workspace_size(C.byref(d))
    if not lib.has_plan:
        return [ws] + [-1] * len(PLAN_FIELDS)
    g = plan(lib, d)
    return [ws] + [getattr(g, f) for f in PLAN_FIELDS]


def rows(lib):
    return [row(lib, descriptor(**p)) for p in problems()]


def table(path=None):
    """int64 [len(ENVS), len(problems()), len(COLUMNS)] of the library at `path`.  Needs a process that has not set either knob itself:
    the in-process rows are those of the defaults."""
    assert not any(k in os.environ for k in KNOBS), "the PF_ATTN_BWD_* knobs must be unset here"
    path = path or _lib.LIB_PATH
    children = []
    for env in ENVS[1:]:                           # (all started first: they run beside the in-process rows)
        e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.dirname(os.path.abspath(__file__)), **env)
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=e, stdout=subprocess.PIPE, text=True))
    out = [rows(load(path))]
    for env, ch in zip(ENVS[1:], children):
        text, _ = ch.communicate(timeout=300)
        assert ch.returncode == 0, "child for %s failed" % (env,)
        out.append(json.loads(text.strip().split("\n")[-1]))
    return np.array(out, dtype=np.int64)


def plan_class(p, g):
    """The launch line of pf_attention_bwd that plan fields g (a mapping) of problem p name: (kernel, D, split)."""
    return (g["kernel"], p["D"], g["qsplit"] > 1)


# every launch line of the dispatch: three kernel pairs x two head dims, the LDS pairs also split (k_attn_bwd_reduce follows those)
CLASSES = tuple((k, D, False) for k in (0, 1, 2) for D in (32, 64)) + ((2, 32, True), (2, 64, True))


if __name__ == "__main__":
    print(json.dumps(rows(load(sys.argv[1]))))
