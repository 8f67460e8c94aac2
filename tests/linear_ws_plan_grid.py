"""The fixed grid of pf_linear_ws problems behind tests/golden/linear_ws_plans.npz (tools/make_golden_linear_ws_plans.py writes it,
tests/test_linear_ws_plans.py reruns it).  Per problem and per setting of the seven knobs: the ROUTE -- which launcher the front end
of the problem's mode (ops.linear / linear_qkv / linear_ln / linear_vt, called the way engine.py calls them, on tensors that carry only
shape, dtype and strides) reaches, and with which mode -- pf_linear_ws_supported, and the whole pf_lws_plan.  The knobs are read once
per process, so every setting is a fresh child process (this file run as a script).  The child imports panfusion_amd from the tree it
is pointed at and touches only names that trees from before pf_linear_ws_plan have too: the same harness records the routes of an older
checkout.  Host arithmetic only: no GPU is opened."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L16, F32, GEGLU, QKV, F32_LN, VT = range(6)
KNOBS = ("PF_LINEAR_WS", "PF_LINEAR_WS_K640", "PF_LINEAR_WS_K1280", "PF_LINEAR_VT", "PF_LINEAR_LN", "PF_LINEAR_WS_MIN_ROWS", "PF_LWS_COUNTED")
ENVS = ({}, {"PF_LINEAR_WS": "0"}, {"PF_LINEAR_WS_K640": "0"}, {"PF_LINEAR_WS_K1280": "0"}, {"PF_LINEAR_VT": "0"}, {"PF_LINEAR_LN": "0"},
        {"PF_LINEAR_WS_MIN_ROWS": "4096"}, {"PF_LWS_COUNTED": "0"})
PLAN_FIELDS = ("supported", "preferred", "k", "chb", "tile_tokens", "nblocks", "ntiles", "splits_per_xcd", "flat_splits", "counted")
COLUMNS = ("route", "supported_query") + PLAN_FIELDS
# route: 0 = the front end returned None (the caller takes another path), 1 = ops.conv_gemm, 2 = ops.linear_t, 10 + mode = ops.linear_ws
ROUTE_NONE, ROUTE_CONV, ROUTE_T, ROUTE_WS = 0, 1, 2, 10


def prob(tag, M, N, K, mode, n_batch=1, a_ld=None, dtype="bf16"):
    """n_batch: batches of the transposed outputs (QKV, VT: rows_per_batch = M // n_batch); a_ld: row stride of x (default K)."""
    return dict(tag=tag, M=M, N=N, K=K, mode=mode, n_batch=n_batch, a_ld=a_ld or K, dtype=dtype)


# every pf_linear_ws launch of the benchmark step, both branches, all three levels (profiles/r6_final_shapes.txt, r6_final_shapes_cfg4.txt):
# (M, N, K, mode, batches)
STEP = ((10240, 10240, 1280, GEGLU, 1), (163840, 2560, 320, GEGLU, 1), (40960, 5120, 640, GEGLU, 1), (163840, 320, 320, F32_LN, 1),
        (163840, 960, 320, QKV, 40), (10240, 2560, 1280, L16, 1), (40960, 1280, 640, L16, 1), (163840, 320, 320, L16, 1),
        (10240, 1280, 1280, VT, 40), (40960, 640, 640, VT, 40), (10240, 1280, 1280, L16, 1), (40960, 640, 640, L16, 1),
        (16384, 2560, 320, GEGLU, 1), (16384, 960, 320, QKV, 2), (40960, 2560, 320, GEGLU, 1), (10240, 5120, 640, GEGLU, 1),
        (40960, 320, 320, F32_LN, 1), (40960, 960, 320, QKV, 2), (10240, 1280, 640, L16, 1),
        (16384, 5120, 640, GEGLU, 1), (65536, 2560, 320, GEGLU, 1), (65536, 320, 320, F32_LN, 1), (65536, 960, 320, QKV, 16),
        (16384, 1280, 640, L16, 1), (65536, 320, 320, L16, 1), (16384, 640, 640, VT, 16), (16384, 640, 640, L16, 1))
# linears of the step that stay on the tile kernel: too few rows, or a (K, mode) the kernel does not have
STEP_TILE = ((16384, 320, 320, F32_LN, 1), (16384, 320, 320, L16, 1), (2560, 1280, 1280, L16, 1), (2560, 10240, 1280, GEGLU, 1),
             (2560, 1280, 1280, VT, 40), (163840, 320, 1280, F32, 1), (40960, 640, 2560, F32, 1), (40960, 640, 640, F32, 1),
             (10240, 1280, 1280, F32, 1), (4096, 2560, 320, GEGLU, 1))
# tests/test_gpu_kernels.py: test_linear_ws_transposed_output (n_batch, nk, N, K), ..._is_bit_reproducible_under_contention (M, N, K, mode)
VT_TEST = ((40, 1024, 640, 640), (40, 256, 1280, 1280), (1, 20480, 640, 640), (3, 96, 128, 640), (2, 48, 256, 1280), (1, 81920, 320, 320),
           (2, 192, 640, 320))
CONTENTION_TEST = ((10240, 1280, 1280, VT), (40960, 640, 640, VT), (10240, 1280, 1280, L16), (10240, 10240, 1280, GEGLU),
                   (40960, 1280, 640, L16), (40960, 5120, 640, GEGLU), (163840, 960, 320, QKV), (163840, 320, 320, F32))


def problems():
    """Every problem of the grid (the order is part of the fixture)."""
    out = [prob("step", *s) for s in STEP] + [prob("step_tile", *s) for s in STEP_TILE]
    # the shapes the GPU tests launch
    for M in (64 * 37 + 40, 64, 64 * 300):                                        # test_linear_ws_modes_vs_fp32
        out += [prob("gpu_k320", M, N, 320, mode) for N, mode in ((320, L16), (320, F32), (640, L16), (2560, L16), (2560, GEGLU))]
    for M in (32 * 37 + 20, 32, 32 * 1300):                                       # test_linear_ws_k640_vs_fp32
        out += [prob("gpu_k640", M, N, 640, mode) for N, mode in ((256, L16), (1280, L16), (5120, GEGLU), (640, L16))]
    out += [prob("gpu_k640", 1 << 16, 640, 640, F32), prob("gpu_k640", 1 << 16, 320, 640, L16)]
    for M in (16 * 37 + 9, 16, 10240):                                            # test_linear_ws_k1280_vs_fp32
        out += [prob("gpu_k1280", M, N, 1280, mode) for N, mode in ((128, L16), (1280, L16), (2560, L16), (10240, GEGLU))]
    out += [prob("gpu_k1280", 1 << 16, 1280, 1280, F32)]
    out += [prob("gpu_vt", nb * nk, N, K, VT, nb) for nb, nk, N, K in VT_TEST]
    out += [prob("gpu_contention", M, N, K, mode, 40) for M, N, K, mode in CONTENTION_TEST]
    out += [prob("gpu_ln", M, 320, 320, F32_LN) for M in (64 * 37 + 40, 64 * 600)]   # test_linear_ws_with_layernorm_epilogue
    for nb, nk in ((3, 1024), (2, 64), (10, 4096)):                                # test_linear_ws_qkv_with_transposed_values
        out += [prob("gpu_qkv", nb * nk, 960, 320, QKV, nb), prob("gpu_qkv", nb * nk, 320, 320, F32)]
    # ---- the edges of every rule
    for M in (8191, 8192):                                                        # PF_LINEAR_WS_MIN_ROWS (4095 / 4096 for its other setting)
        out += [prob("min_rows", M, 2560, 320, GEGLU), prob("min_rows", M, 1280, 640, L16), prob("min_rows", M, 1280, 1280, L16)]
    out += [prob("min_rows", M, 2560, 320, GEGLU) for M in (4095, 4096)]
    for M in (32767, 32768, 16383, 16384):                                        # one channel block at K = 320: 4 x as many rows
        out += [prob("min_rows_n320", M, 320, 320, mode) for mode in (L16, F32, F32_LN)]
    out += [prob("min_tile", M, 640, 320, L16) for M in (63, 64)] + [prob("min_tile", M, 1280, 640, L16) for M in (31, 32)]
    out += [prob("min_tile", M, 1280, 1280, L16) for M in (15, 16)]
    # every nblocks at K = 640 with 128-channel workgroups: the XCD-grouped grid against the flat one (8 * (32 / nblocks) * nblocks >= 200)
    out += [prob("nblocks_640", 40960, 128 * nb, 640, VT, 40) for nb in range(1, 34)]
    out += [prob("nblocks_640", 40960, 128 * nb, 640, L16) for nb in range(1, 34, 2)]
    out += [prob("nblocks_1280", 10240, 128 * nb, 1280, L16) for nb in (33, 80, 128, 129)]
    out += [prob("nblocks_320", 163840, 320 * nb, 320, L16) for nb in (11, 20, 32, 33)]   # (11, 20: the flat grid)
    out += [prob("nblocks_256", 40960, 256 * nb, 640, GEGLU) for nb in (32, 33)]
    out += [prob("n640_k640", 40960, 640, 640, mode, 40) for mode in range(6)]      # N a multiple of 128 but not of 256, each mode
    # batches of a transposed output that are whole tiles, or half a tile short of it
    out += [prob("batch", 40 * nk, 960, 320, QKV, 40) for nk in (4096 - 64, 4096 - 32)]
    out += [prob("batch", 40 * nk, 320, 320, VT, 40) for nk in (4096 - 64, 4096 - 32)]
    out += [prob("batch", 40 * nk, 640, 640, VT, 40) for nk in (1024 - 32, 1024 - 16)]
    out += [prob("batch", 40 * nk, 1280, 1280, VT, 40) for nk in (256 - 16, 256 - 8)]
    out += [prob("batch", 8200, 640, 640, VT, 3), prob("batch", 8200, 960, 320, QKV, 3)]   # rows that are no whole batches
    # the layout of x: a row stride that is not a multiple of 8, a column-sliced view, fp32
    out += [prob("a_ld", 163840, 960, 320, QKV, 40, a_ld=324), prob("a_ld", 163840, 2560, 320, GEGLU, a_ld=324),
            prob("a_ld", 40960, 640, 640, VT, 40, a_ld=644), prob("a_ld", 163840, 320, 320, F32_LN, a_ld=640),
            prob("a_ld", 163840, 320, 320, L16, a_ld=960)]
    out += [prob("fp32", 163840, 320, 320, mode, dtype="f32") for mode in (L16, F32, F32_LN)] + [prob("fp32", 40960, 640, 640, VT, 40, dtype="f32")]
    out += [prob("fp16", 163840, 960, 320, QKV, 40, dtype="f16"), prob("fp16", 10240, 10240, 1280, GEGLU, dtype="f16")]
    # each (K, mode) pair the kernel does not have, and a K it does not have
    out += [prob("unsupported", 40960, N, 640, mode, 40) for N, mode in ((1280, F32), (1920, QKV), (960, QKV), (320, F32_LN), (1280, F32_LN))]
    out += [prob("unsupported", 10240, N, 1280, mode, 40) for N, mode in ((1280, F32), (3840, QKV), (960, QKV), (320, F32_LN), (1280, F32_LN))]
    out += [prob("unsupported", 163840, N, 320, mode, 40) for N, mode in ((640, QKV), (1280, QKV), (640, F32_LN), (300, L16))]
    out += [prob("unsupported", 40960, 960, 960, mode, 40) for mode in (L16, F32, GEGLU, VT)]
    return out


def rows_per_batch(p):
    return p["M"] // p["n_batch"] if p["mode"] in (QKV, VT) else 0


def plan_class(p, g):
    """(k, chb, mode): the k_linear_ws instantiation that plan fields g (a mapping) of problem p name."""
    return (int(g["k"]), int(g["chb"]), p["mode"])


# every launch line of the dispatch
CLASSES = tuple((320, 320, m) for m in range(6)) + ((640, 256, L16), (640, 256, GEGLU), (640, 128, L16), (640, 128, VT),
                                                    (1280, 128, L16), (1280, 128, GEGLU), (1280, 128, VT))


# ------------------------------------------------------------------------------------------------ the child: one tree, one setting
def _rows(root):
    sys.path.insert(0, root)
    import ctypes as C

    import torch
    from panfusion_amd import _lib, ops
    lib = _lib.lib()
    reached = []
    ops.linear_ws = lambda x, w, mode, **kw: reached.append(ROUTE_WS + mode) or ((x, w) if mode in (QKV, F32_LN) else x)
    ops.conv_gemm = lambda *a, **kw: reached.append(ROUTE_CONV) or a[0]
    ops.linear_t = lambda *a, **kw: reached.append(ROUTE_T) or a[0]
    has_plan = hasattr(lib, "pf_linear_ws_plan")
    meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, device="meta", dtype=dtype)
    out = []
    for p in problems():
        M, N, K, mode, nb = p["M"], p["N"], p["K"], p["mode"], p["n_batch"]
        dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[p["dtype"]]
        x = torch.empty_strided((M, K), (p["a_ld"], 1), device="meta", dtype=dtype)
        w, b = meta(N, K, dtype=dtype), meta(N)
        del reached[:]
        if mode == L16:
            ops.linear(x, w)                                                     # engine.self_qkv / _attend: q | k, to_q
        elif mode == F32:
            ops.linear(x, w, bias=b, residual=meta(M, N))                        # engine._attend: to_out on the fp32 stream
        elif mode == GEGLU:
            ops.linear(x, w, bias=b, geglu=True)                                 # engine.run_transformer: FF1
        elif mode == QKV:
            ops.linear_qkv(x, w, nb)                                             # engine.self_qkv
        elif mode == F32_LN:
            ops.linear_ln(x, w, b, meta(M, N), meta(N), meta(N), 1e-5)           # engine._attend: to_out + the next LayerNorm
        else:
            ops.linear_vt(x, w, nb)                                              # engine.self_qkv
        assert len(reached) <= 1, (p, reached)
        row = [reached[0] if reached else ROUTE_NONE, lib.pf_linear_ws_supported(M, N, K, mode)]
        if has_plan:
            d, g = _lib.LinearWsDesc(), _lib.LwsPlan()
            d.M, d.N, d.K, d.mode, d.a_ld, d.dtype, d.rows_per_batch = M, N, K, mode, p["a_ld"], ops.dt(dtype), rows_per_batch(p)
            assert lib.pf_linear_ws_plan(C.byref(d), C.byref(g)) == 0
            row += [getattr(g, f) for f in PLAN_FIELDS]
        else:
            row += [-1] * len(PLAN_FIELDS)
        out.append(row)
    return out


def table(root=ROOT):
    """int64 [len(ENVS), len(problems()), len(COLUMNS)] of the tree at `root` and the library built in it (the plan columns -1 for a
    library without pf_linear_ws_plan)."""
    children = []
    for env in ENVS:
        e = {k: v for k, v in os.environ.items() if k not in KNOBS + ("PF_HIP_LIB",)}
        e.update(env)
        children.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), root], env=e, stdout=subprocess.PIPE, text=True))
    out = []
    for env, ch in zip(ENVS, children):
        text, _ = ch.communicate(timeout=600)
        assert ch.returncode == 0, "child for %s failed" % (env,)
        out.append(json.loads(text.strip().split("\n")[-1]))
    return np.array(out, dtype=np.int64)


if __name__ == "__main__":
    print(json.dumps(_rows(sys.argv[1])))
