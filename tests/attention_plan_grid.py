"""The fixed grid of pf_attention problems behind tests/golden/attention_plans.npz (tools/make_golden_attention_plans.py writes it,
tests/test_attention_plans.py reruns it): descriptors on fake, never dereferenced pointers, pf_attention_workspace_size and the
whole pf_attn_plan of each, under every setting of the PF_ATTENTION_* knobs that changes the dispatch.  The knobs the planner reads
per call are switched in this process; the ones it reads once per process each get a child process (this file run as a script).
Host arithmetic only: no GPU is opened."""
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

LIVE_KNOBS = ("PF_ATTENTION_PP", "PF_ATTENTION_SPLIT")
LIVE_ENVS = ({}, {"PF_ATTENTION_SPLIT": "0"}, {"PF_ATTENTION_PP": "1"}, {"PF_ATTENTION_PP": "2"})
PROCESS_KNOBS = ("PF_ATTENTION_OCC", "PF_ATTENTION_OCC32", "PF_ATTENTION_MSUM", "PF_ATTENTION_MSUM32", "PF_ATTENTION_IMPL",
                 "PF_ATTENTION_SPLIT_MIN_TILES", "PF_ATTENTION_PP_ROLE", "PF_ATTENTION_PP_PRIO", "PF_ATTENTION_XCD", "PF_ATTENTION_STEADY2")
PROCESS_ENVS = ({"PF_ATTENTION_OCC": "2"}, {"PF_ATTENTION_MSUM": "0"}, {"PF_ATTENTION_OCC32": "5"}, {"PF_ATTENTION_OCC32": "3"},
                {"PF_ATTENTION_OCC32": "3", "PF_ATTENTION_MSUM32": "1"}, {"PF_ATTENTION_IMPL": "direct"}, {"PF_ATTENTION_SPLIT_MIN_TILES": "4"})
ENVS = LIVE_ENVS + PROCESS_ENVS
PLAN_FIELDS = tuple(f for f, _ in _lib.AttnPlan._fields_)
COLUMNS = ("workspace_size",) + PLAN_FIELDS
OPAD = 8                 # canary columns on either side of an output in tests/test_gpu_attention_bounds.py


def prob(tag, B, H, D, nq, nk, bias=False, lse=False, o_ld=None, vt_ld=None, wide=1):
    """wide: q and k sit in one buffer of wide * H * D columns (the fused q | k projection)."""
    return dict(tag=tag, B=B, H=H, D=D, nq=nq, nk=nk, bias=bias, lse=lse, o_ld=o_ld, vt_ld=vt_ld, wide=wide)


def fwd_case_problem(c):
    """FWD_CASES entry -> the descriptor test_gpu_attention_bounds.py launches (output inside a wider buffer, its own vt_ld)."""
    return prob("fwd:" + c.name, c.B, c.H, c.D, c.nq, c.nk, bias=c.bias, lse=c.lse, o_ld=c.H * c.D + 2 * OPAD, vt_ld=c.vt_ld,
                wide=2 if c.fused else 1)


SPLIT_TEST = ((2, 4, 256, 4096), (1, 10, 128, 1280), (2, 3, 200, 2084), (1, 2, 96, 1156))            # test_attention_split_key_range
PP_TEST = ((2, 5, 64, 512, 512), (1, 3, 64, 300, 1000), (1, 2, 64, 64, 136), (3, 2, 64, 257, 4096),
           (2, 5, 64, 512, 512), (1, 3, 64, 300, 1152), (1, 2, 64, 33, 256), (3, 2, 64, 257, 4096))  # test_pingpong_attention_kernels
# the attention launches of the benchmark step (profiles/r4_final_shapes.txt): (B, H, D, nq, nk, bias)
STEP = ((40, 5, 64, 4096, 4096, 0), (2, 5, 64, 8192, 8192, 0), (40, 10, 64, 1024, 1024, 0), (2, 10, 64, 2048, 2048, 0),
        (40, 20, 64, 256, 256, 0), (2, 20, 64, 512, 512, 0), (40, 20, 64, 64, 64, 0), (2, 20, 64, 128, 128, 0),
        (40, 5, 64, 4096, 77, 0), (2, 5, 64, 8192, 77, 0), (40, 10, 64, 1024, 77, 0), (2, 10, 64, 2048, 77, 0),
        (40, 20, 64, 256, 77, 0), (2, 20, 64, 512, 77, 0), (40, 20, 64, 64, 77, 0), (2, 20, 64, 128, 77, 0),
        (2, 10, 32, 2048, 20480, 1), (2, 20, 32, 2048, 20480, 1), (2, 10, 32, 20480, 2048, 1), (2, 20, 32, 20480, 2048, 1),
        (2, 20, 32, 512, 5120, 1), (2, 40, 32, 512, 5120, 1), (2, 20, 32, 5120, 512, 1), (2, 40, 32, 5120, 512, 1),
        (2, 40, 32, 128, 1280, 1), (2, 40, 32, 1280, 128, 1))


def problems():
    """Every problem of the grid (the order is part of the fixture)."""
    out = [fwd_case_problem(c) for c in M.FWD_CASES]
    out += [prob("split_test", B, H, 32, nq, nk, bias=True) for B, H, nq, nk in SPLIT_TEST]
    out += [prob("pp_test", *cfg) for cfg in PP_TEST]
    out += [prob("step", B, H, D, nq, nk, bias=bool(b), wide=1 if b or nk == 77 else 2) for B, H, D, nq, nk, b in STEP]
    # the split rule's edges: 972 / 973 query blocks against 1024 slots (blocks * 20 < / >= slots * 19), 15 / 16 / 17 key tiles, an
    # output whose rows are not 16-byte aligned, an lse, a V^T layout that takes the no-LDS kernel
    out += [prob("split_edge", 9, 27, 32, 512, 2048, bias=True), prob("split_edge", 1, 139, 32, 896, 2048, bias=True)]
    out += [prob("split_edge", 1, 2, 32, 128, nk, bias=True) for nk in (960, 1024, 1088)]
    out += [prob("split_edge", 1, 2, 32, 128, 2048, bias=True, o_ld=68), prob("split_edge", 1, 2, 32, 128, 2048, bias=True, lse=True),
            prob("split_edge", 1, 2, 32, 128, 2048, bias=True, vt_ld=2052), prob("split_edge", 1, 2, 32, 128, 2048)]
    # the MSUM edge and the ping-pong kernels' key-count conditions (D = 64, no bias), with and without an lse
    out += [prob("d64_edge", 1, 2, 64, 256, nk) for nk in (120, 128, 132, 136, 255, 256, 384)]
    out += [prob("d64_edge", 1, 2, 64, 256, nk, lse=True) for nk in (136, 256)]
    out += [prob("d64_edge", 1, 2, 64, 256, 256, bias=True), prob("d64_edge", 1, 2, 64, 256, 256, vt_ld=260)]
    return out


def descriptor(tag, B, H, D, nq, nk, bias, lse, o_ld, vt_ld, wide):
    d = _lib.AttnDesc()
    d.q, d.k, d.vt, d.out = 0x10000, 0x20000, 0x30000, 0x40000
    d.dtype, d.B, d.H, d.D, d.nq, d.nk = _lib.PF_BF16, B, H, D, nq, nk
    d.q_ld = d.k_ld = wide * H * D
    d.vt_ld = vt_ld or (nk + 31) // 32 * 32
    d.o_ld = o_ld or H * D
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = nq * d.q_ld, (nk + 64) * d.k_ld, H * D * d.vt_ld, nq * d.o_ld
    d.scale = D ** -0.5
    if bias:
        d.bias, d.bias_ld, d.flags, d.flags_ld = 0x50000, nk, 0x60000, (nk + 31) // 32
    if lse:
        d.lse = 0x70000
    return d


def load(path=None):
    """The attention queries of the library at `path` (default: the one panfusion_amd uses), bound directly: a library from before
    pf_attention_plan existed loads too and has has_plan False."""
    import torch  # noqa: F401  (the library resolves the HIP runtime torch ships, as panfusion_amd._lib does)
    lib = C.CDLL(path or _lib.LIB_PATH)
    lib.pf_attention_workspace_size.restype, lib.pf_attention_workspace_size.argtypes = _lib.SIGNATURES["pf_attention_workspace_size"]
    lib.has_plan = hasattr(lib, "pf_attention_plan")
    if lib.has_plan:
        lib.pf_attention_plan.restype, lib.pf_attention_plan.argtypes = _lib.SIGNATURES["pf_attention_plan"]
    return lib


def plan(lib, d):
    g = _lib.AttnPlan()
    assert lib.pf_attention_plan(C.byref(d), C.byref(g)) == 0
    return g


def row(lib, d):
    """One fixture row: COLUMNS of descriptor d (the plan columns -1 for a library without pf_attention_plan)."""
    ws = lib.pf_attention_workspace_size(C.byref(d))
    if not lib.has_plan:
        return [ws] + [-1] * len(PLAN_FIELDS)
    g = plan(lib, d)
    return [ws] + [getattr(g, f) for f in PLAN_FIELDS]


class live_env:
    """The planner's per-call knobs set to exactly `env` (the library reads them with getenv on every query)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in LIVE_KNOBS}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in LIVE_KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.saved.items() if v is not None})


def rows(lib):
    return [row(lib, descriptor(**p)) for p in problems()]


def table(path=None):
    """int64 [len(ENVS), len(problems()), len(COLUMNS)] of the library at `path`.  Needs a process that has not set any of
    PROCESS_KNOBS itself: the in-process rows are those of the defaults."""
    assert not any(k in os.environ for k in PROCESS_KNOBS), "the once-per-process PF_ATTENTION_* knobs must be unset here"
    path = path or _lib.LIB_PATH
    children = []
    for env in PROCESS_ENVS:                       # (all started first: they run beside the in-process rows)
        e = {k: v for k, v in os.environ.items() if k not in LIVE_KNOBS}
        e.update(env, PYTHONPATH=ROOT + os.pathsep + os.path.dirname(os.path.abspath(__file__)))
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=e, stdout=subprocess.PIPE, text=True))
    lib = load(path)
    out = []
    for env in LIVE_ENVS:
        with live_env(env):
            out.append(rows(lib))
    for env, ch in zip(PROCESS_ENVS, children):
        text, _ = ch.communicate(timeout=300)
        assert ch.returncode == 0, "child for %s failed" % (env,)
        out.append(json.loads(text.strip().split("\n")[-1]))
    return np.array(out, dtype=np.int64)


def plan_class(p, g):
    """The launch arm of pf_attention that plan fields g (a mapping) of problem p name: (kernel, D, bias, pipelined, occupancy, msum,
    split).  The no-LDS and ping-pong kernels have one instantiation per D whatever the bias."""
    if g["kernel"] != 1:
        return (g["kernel"], p["D"], False, 0, 0, 0, False)
    return (1, p["D"], bool(p["bias"]), g["pipelined"], g["occupancy"], g["msum"], g["splits"] > 1)


# every launch line of the dispatch: k_attention x 2, the two ping-pong kernels, the eleven k_attention_lds instantiations, two of them
# also split (the k_attention_merge launch follows those)
CLASSES = ((0, 64, False, 0, 0, 0, False), (0, 32, False, 0, 0, 0, False), (2, 64, False, 0, 0, 0, False), (3, 64, False, 0, 0, 0, False),
           (1, 64, True, 1, 2, 0, False), (1, 64, False, 1, 2, 0, False), (1, 64, False, 0, 3, 1, False), (1, 64, False, 0, 3, 0, False),
           (1, 32, True, 0, 4, 0, True), (1, 32, True, 0, 5, 0, True), (1, 32, True, 0, 4, 0, False), (1, 32, True, 0, 5, 0, False),
           (1, 32, True, 1, 3, 1, False), (1, 32, True, 1, 3, 0, False),
           (1, 32, False, 0, 4, 0, False), (1, 32, False, 0, 5, 0, False), (1, 32, False, 1, 3, 0, False))


if __name__ == "__main__":
    print(json.dumps(rows(load(sys.argv[1]))))
