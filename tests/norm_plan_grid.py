"""The fixed grid of GroupNorm / LayerNorm problems behind tests/golden/norm_plans.npz (tools/make_golden_norm_plans.py writes it,
tests/test_norm_plans.py reruns it, tests/test_norm_bounds_cpu.py holds tests/norm_model.py against it).  Three tables -- statistics
(pf_groupnorm_plan), backward (pf_groupnorm_bwd_plan) and LayerNorm (pf_layernorm_plan) -- each per problem and per setting of
PF_GN_DIRECT_MAX: the size queries that existed before the planner, the planner's status and the whole plan.  The knob is read once per
process, so every setting is a fresh child process (this file run as a script).  The child imports panfusion_amd from the tree it is
pointed at and, for the query columns, touches only names that trees from before the planner have too: the same harness records an older
checkout.  Host arithmetic only: no GPU is opened."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = 0, 1, 2
DIRECT, TWO_STAGE, FROM_PARTIALS = 1, 2, 3
KNOBS = ("PF_GN_DIRECT_MAX",)
ENVS = ({}, {"PF_GN_DIRECT_MAX": "0"})
GN_FIELDS = ("arm", "partials_refused", "ppc", "nchunks", "pix_par", "lds_bytes", "gpb", "pairs_per_block", "slices",
             "grid_x", "grid_y", "grid2_x", "grid2_y", "workspace_bytes")
BWD_FIELDS = ("ppc", "chunks", "pix_par", "bwd_lds_bytes", "param_lds_bytes", "partial_grid_x", "partial_grid_y", "finalize_grid_x",
              "apply_grid_x", "apply_grid_y", "bwd_workspace_bytes", "param_partial_bytes", "param_workspace_bytes")
LN_FIELDS = ("rows_per_wave", "grid_x", "bwd_parts")
# the first columns of each table are the queries a tree from before the planner answers too (the fixture's `*_parent` arrays)
GN_COLUMNS = ("ws_query", "status") + GN_FIELDS
BWD_COLUMNS = ("bwd_ws_query", "param_ws_query", "status") + BWD_FIELDS
LN_COLUMNS = ("parts_query", "status") + LN_FIELDS
N_PARENT = dict(gn=1, bwd=2, ln=1)
COLUMNS = dict(gn=GN_COLUMNS, bwd=BWD_COLUMNS, ln=LN_COLUMNS)


def gn(tag, n, hw, c0, c1, groups, dtype=BF16, rows0=0, rows1=0):
    """rows0 / rows1: rows per part of the moments attached to the sources (0: none)."""
    return dict(tag=tag, n=n, hw=hw, c0=c0, c1=c1, groups=groups, dtype=dtype, rows0=rows0, rows1=rows1)


def bwd(tag, n, hw, c0, c1, groups):
    """groups = 0: pf_groupnorm_param_grads alone."""
    return dict(tag=tag, n=n, hw=hw, c0=c0, c1=c1, groups=groups)


def ln(tag, rows, C):
    return dict(tag=tag, rows=rows, C=C)


# tests/norm_model.py GN_CASES, PART_CASES (n, hw, c0, rows0, c1, rows1, groups) and LN_CASES, restated
MODEL_GN = ((3, 408, 64, 32, 32), (1, 64, 1280, 1280, 32), (2, 1, 64, 0, 32), (1, 4099, 320, 0, 32), (1, 16411, 64, 0, 32),
            (1, 421, 2560, 0, 32), (2, 4096, 192, 128, 32), (40, 1024, 128, 0, 32), (40, 8190, 16, 0, 4), (2, 96, 64, 32, 32),
            (1, 40, 64, 0, 32), (1, 64 * 132, 320, 0, 32), (1, 65 * 132, 320, 0, 32))
MODEL_PART = ((2, 64, 2560, 8, 0, 0, 32), (2, 256, 1280, 16, 0, 0, 32), (2, 1024, 128, 16, 0, 0, 32), (2, 1024, 128, 4, 0, 0, 32),
              (2, 1024, 128, 1, 0, 0, 32), (2, 256, 192, 64, 128, 16, 32), (2, 64, 96, 8, 0, 0, 12), (1, 64, 2560, 8, 0, 0, 8),
              (2, 64, 96, 8, 0, 0, 32), (2, 100, 128, 8, 0, 0, 32))
MODEL_LN = tuple((r, C) for r in (4096, 4099) for C in (8, 64, 320, 512)) + tuple((r, C) for r in (1, 111, 4097) for C in (8, 520, 1280, 2048))
# GroupNorm calls of the denoiser and of the VAE: (n_img, hw, c0, c1) at 32 groups -- views 8 x 32^2 .. 4^2, panorama 2 x (32 x 64) .. ,
# skip concatenations, the 512^2 VAE levels
STEP_GN = ((8, 1024, 320, 0), (8, 1024, 320, 320), (8, 1024, 640, 320), (8, 256, 640, 0), (8, 256, 640, 640), (8, 256, 1280, 640),
           (8, 64, 1280, 0), (8, 64, 1280, 1280), (8, 16, 1280, 0), (8, 16, 1280, 1280), (2, 2048, 320, 0), (2, 2048, 320, 320),
           (2, 512, 640, 0), (2, 512, 1280, 640), (2, 128, 1280, 1280), (2, 32, 1280, 0), (1, 4096, 512, 0), (1, 16384, 512, 0),
           (1, 65536, 256, 0), (1, 262144, 128, 0), (4, 262144, 128, 0))


def gn_problems():
    """Every statistics problem of the grid (the order is part of the fixture)."""
    out = [gn("model_gn", n, hw, c0, c1, g, dtype=(BF16, F16, F32)[i % 3]) for i, (n, hw, c0, c1, g) in enumerate(MODEL_GN)]
    out += [gn("model_part", n, hw, c0, c1, g, F32, r0, r1) for n, hw, c0, r0, c1, r1, g in MODEL_PART]
    out += [gn("step", n, hw, c0, c1, 32, F16) for n, hw, c0, c1 in STEP_GN]
    out += [gn("step", n, hw, c0, c1, 32, F32) for n, hw, c0, c1 in STEP_GN[:4]]
    # ---- the edges of the arm rule: hw * cpg against 32768, n * hw * C against 4 Mi
    out += [gn("arm_hwcpg", 1, hw, 256, 0, 32) for hw in (4096, 4097)] + [gn("arm_hwcpg", 1, 1024, C, 0, 32) for C in (1024, 1056)]
    out += [gn("arm_cap", n, 1024, 1024, 0, 32) for n in (4, 5)] + [gn("arm_cap", n, 4096, 256, 0, 32) for n in (4, 5)]
    out += [gn("arm_cap", 16, 1024, 128, 128, 32), gn("arm_cap", 16, 1025, 128, 128, 32)]
    # ---- pixels per chunk: the clamp at 8, at 64, the hw / 256 floor, hw itself (an image of fewer than 8 pixels, two-stage through the cap)
    out += [gn("ppc_8", 1, 1025, 2560, 0, 32), gn("ppc_8", 7, 2048, 320, 0, 32), gn("ppc_mid", 9, 2048, 320, 0, 32)]
    out += [gn("ppc_64", 65, 2048, 320, 0, 32), gn("ppc_64", 40, 16384, 64, 0, 32), gn("ppc_floor", 1, 16385, 64, 0, 32)]
    out += [gn("ppc_floor", 1, 2049, 320, 0, 32), gn("ppc_hw", 1000, 5, 1024, 0, 32), gn("ppc_hw", 3000, 7, 256, 0, 32)]
    # ---- the staging layout: C / 8 octets over 256 threads (pix_par 128 .. 1, two octet rounds from C = 2056), the 64 KiB limit
    out += [gn("pix_par", 1, 40000, C, 0, g) for C, g in ((8, 1), (16, 2), (24, 3), (320, 32), (1024, 32), (2040, 1), (2048, 32), (2056, 1))]
    out += [gn("lds", 1, 200, C, 0, 32) for C in (8192, 8320)] + [gn("lds", 100, 2, 8320, 0, 32)]     # (the last: direct, no staging)
    # ---- moments: groups per block by parts per image (32 | 33, 128 | 129, 512 | 513), halved by the pair cap, ragged last blocks, refusals
    out += [gn("gpb", 2, 16 * ppi, 128, 0, 32, F32, 16) for ppi in (32, 33, 128, 129, 512, 513)]
    out += [gn("gpb_cap", 1, 64, C, 0, g, F32, 8) for C, g in ((2560, 8), (2560, 2), (1024, 1), (2048, 1), (2064, 1), (4128, 2))]
    out += [gn("ragged", 2, 64, 96, 0, 12, F32, 8), gn("ragged", 2, 2048, 160, 0, 10, F32, 16), gn("ragged", 1, 64, 24, 0, 3, F32, 64)]
    out += [gn("two_sources", 2, 256, 192, 128, 32, F32, 64, 16), gn("two_sources", 2, 256, 192, 128, 32, F32, 16, 64),
            gn("two_sources", 2, 256, 192, 128, 32, F32, 64, 0), gn("two_sources", 2, 256, 190, 130, 32, F32, 64, 16)]
    out += [gn("part_refused", 2, 64, 96, 0, 32, F32, 8), gn("part_refused", 2, 100, 128, 0, 32, F32, 8),
            gn("part_refused", 2, 256, 192, 128, 32, F32, 64, 48), gn("part_refused", 2, 64, 95, 97, 32, F32, 8, 8)]       # (the last: an odd source, which the statistics pass refuses too)
    # ---- refused outright: sizes, channels, groups, dtype
    out += [gn("refused", 0, 64, 64, 0, 32), gn("refused", 1, 0, 64, 0, 32), gn("refused", 1, 64, 64, 0, 0), gn("refused", 1, 64, 128, 0, 65),
            gn("refused", 1, 64, 60, 0, 30), gn("refused", 1, 64, 60, 68, 32), gn("refused", 1, 64, 64, 0, 24), gn("refused", 1, 64, 64, 0, 32, 3)]
    return out


def bwd_problems():
    out = [bwd("training", n, hw, c0, c1, 32) for n, hw, c0, c1 in ((2, 130, 64, 0), (2, 130, 32, 32), (1, 1024, 320, 0), (4, 256, 640, 640),
                                                                   (4, 64, 1280, 1280), (1, 2048, 320, 320), (8, 16, 1280, 0))]
    # pixels per chunk 64, 32, 16, 8 and the edges between them (16 chunks: hw = 961, 481, 241)
    out += [bwd("ppc", 2, hw, 64, 0, 32) for hw in (1, 8, 130, 240, 241, 300, 480, 481, 600, 960, 961, 1024, 4099)]
    out += [bwd("pix_par", 1, 300, C, 0, g) for C, g in ((8, 1), (64, 8), (2048, 32), (2056, 1))]
    out += [bwd("lds4", 1, 300, C, 0, 32) for C in (4096, 4128, 8192)] + [bwd("lds2", 1, 300, C, 0, 0) for C in (4128, 8192, 8224)]
    out += [bwd("many_groups", 1, 300, C, 0, 1024) for C in (1024, 4096, 8192)]     # more than 512 groups (one channel per group at C = 1024)
    out += [bwd("param_only", n, hw, c0, c1, 0) for n, hw, c0, c1 in ((2, 130, 64, 0), (2, 130, 32, 32), (3, 4099, 320, 0))]
    out += [bwd("refused", 0, 64, 64, 0, 32), bwd("refused", 1, 0, 64, 0, 32), bwd("refused", 1, 64, 60, 0, 30), bwd("refused", 1, 64, 64, 0, 24),
            bwd("refused", 65536, 1, 64, 0, 32), bwd("refused", 1, 64, 0, 64, 32), bwd("refused", 1, 64, 60, 0, 0), bwd("refused", 65536, 1, 64, 0, 0)]
    return out


def ln_problems():
    out = [ln("model_ln", r, C) for r, C in MODEL_LN]
    out += [ln("step", r, C) for r, C in ((163840, 320), (40960, 640), (10240, 1280), (2560, 1280), (16384, 320), (616, 1024))]
    out += [ln("rpw", r, C) for r in (4095, 4096) for C in (504, 512, 520)]
    out += [ln("parts", r, 320) for r in (1, 4, 5, 2044, 2045, 2048, 2049, 10 ** 7)]
    out += [ln("refused", 0, 64), ln("refused", 4, 2056), ln("refused", 4, 60), ln("refused", 4, 0), ln("refused", 4, -8)]
    return out


PROBLEMS = dict(gn=gn_problems, bwd=bwd_problems, ln=ln_problems)

# every class of launch decision the grid must hold a member of: name -> (kind, setting, predicate(problem, row as a mapping))
_cpg = lambda p: (p["c0"] + p["c1"]) // p["groups"]
_elems = lambda p: p["n"] * p["hw"] * (p["c0"] + p["c1"])
_two = lambda g: g["status"] == 0 and g["arm"] == TWO_STAGE
_part = lambda g: g["status"] == 0 and g["arm"] == FROM_PARTIALS
_ppi = lambda p: max(p["hw"] // p["rows0"], p["hw"] // (p["rows1"] or p["rows0"]))
CLASSES = {
    "direct at hw cpg = 32768": ("gn", 0, lambda p, g: g["arm"] == DIRECT and p["hw"] * _cpg(p) == 32768),
    "direct at 4 Mi elements": ("gn", 0, lambda p, g: g["arm"] == DIRECT and _elems(p) == 4 << 20),
    "two-stage through hw cpg": ("gn", 0, lambda p, g: _two(g) and p["hw"] * _cpg(p) > 32768 and _elems(p) <= 4 << 20),
    "two-stage through the 4 Mi cap": ("gn", 0, lambda p, g: _two(g) and p["hw"] * _cpg(p) <= 32768 and _elems(p) > 4 << 20),
    "two-stage by PF_GN_DIRECT_MAX=0": ("gn", 1, lambda p, g: _two(g) and p["hw"] * _cpg(p) <= 32768 and _elems(p) <= 4 << 20),
    "ppc clamped at 8": ("gn", 0, lambda p, g: _two(g) and g["ppc"] == 8 and p["n"] * p["hw"] // 2048 < 8 and p["hw"] > 8),
    "ppc clamped at 64": ("gn", 0, lambda p, g: _two(g) and g["ppc"] == 64 and p["n"] * p["hw"] // 2048 > 64),
    "ppc by the hw / 256 floor": ("gn", 0, lambda p, g: _two(g) and g["ppc"] == -(-p["hw"] // 256) > max(8, min(64, p["n"] * p["hw"] // 2048))),
    "ppc by hw < 8": ("gn", 0, lambda p, g: _two(g) and g["ppc"] == p["hw"] < 8),
    "pix_par 1, two octet rounds": ("gn", 0, lambda p, g: _two(g) and g["pix_par"] == 1 and p["c0"] + p["c1"] > 2048),
    "pix_par 128 > ppc": ("gn", 0, lambda p, g: _two(g) and g["pix_par"] == 128 > g["ppc"]),
    "64 KiB refusal, statistics": ("gn", 0, lambda p, g: g["status"] == 1 and p["tag"] == "lds"),
    "gpb 8": ("gn", 0, lambda p, g: _part(g) and g["gpb"] == 8 and _ppi(p) <= 32),
    "gpb 4": ("gn", 0, lambda p, g: _part(g) and g["gpb"] == 4 and 32 < _ppi(p) <= 128),
    "gpb 2": ("gn", 0, lambda p, g: _part(g) and g["gpb"] == 2 and 128 < _ppi(p) <= 512),
    "gpb 1": ("gn", 0, lambda p, g: _part(g) and g["gpb"] == 1 and _ppi(p) > 512),
    "gpb halved by the pair cap": ("gn", 0, lambda p, g: _part(g) and _ppi(p) <= 32 and g["gpb"] < 8),
    "ragged last block": ("gn", 0, lambda p, g: _part(g) and p["groups"] % g["gpb"] != 0 and g["grid_y"] > 1),
    "two sources, different rows": ("gn", 0, lambda p, g: _part(g) and p["c1"] > 0 and p["rows0"] != p["rows1"]),
    "partials refused, odd channels per group": ("gn", 0, lambda p, g: g["status"] == 0 and g["partials_refused"] == 1 and _cpg(p) % 2 == 1),
    "partials refused, rows": ("gn", 0, lambda p, g: g["status"] == 0 and g["partials_refused"] == 1 and _cpg(p) % 2 == 0 and
                               (p["hw"] % p["rows0"] != 0 or p["hw"] % (p["rows1"] or p["rows0"]) != 0)),
    "backward ppc 64": ("bwd", 0, lambda p, g: g["status"] == 0 and g["ppc"] == 64),
    "backward ppc 32": ("bwd", 0, lambda p, g: g["status"] == 0 and g["ppc"] == 32),
    "backward ppc 16": ("bwd", 0, lambda p, g: g["status"] == 0 and g["ppc"] == 16),
    "backward ppc 8": ("bwd", 0, lambda p, g: g["status"] == 0 and g["ppc"] == 8),
    "64 KiB refusal, backward": ("bwd", 0, lambda p, g: g["status"] == 1 and p["tag"] == "lds4"),
    "64 KiB refusal, parameter gradients": ("bwd", 0, lambda p, g: g["status"] == 1 and p["tag"] == "lds2"),
    "rows per wave 4 at rows = 4096, C = 512": ("ln", 0, lambda p, g: g["rows_per_wave"] == 4 and (p["rows"], p["C"]) == (4096, 512)),
    "rows per wave 1 below 4096 rows": ("ln", 0, lambda p, g: g["rows_per_wave"] == 1 and (p["rows"], p["C"]) == (4095, 512)),
    "rows per wave 1 above C = 512": ("ln", 0, lambda p, g: g["rows_per_wave"] == 1 and (p["rows"], p["C"]) == (4096, 520)),
    "backward parts 1": ("ln", 0, lambda p, g: g["status"] == 0 and g["bwd_parts"] == 1),
    "backward parts in between": ("ln", 0, lambda p, g: g["status"] == 0 and 1 < g["bwd_parts"] < 512 and g["bwd_parts"] == -(-p["rows"] // 4)),
    "backward parts at the cap": ("ln", 0, lambda p, g: g["status"] == 0 and g["bwd_parts"] == 512 and p["rows"] > 2048),
}


def missing_classes(tabs):
    """The names of CLASSES without a member in tables() output `tabs`."""
    out = []
    for name, (kind, e, pred) in CLASSES.items():
        rows = (dict(zip(COLUMNS[kind], tabs[kind][e, i])) for i in range(tabs[kind].shape[1]))
        if not any(pred(p, g) for p, g in zip(PROBLEMS[kind](), rows)):
            out.append(name)
    return out


# ------------------------------------------------------------------------------------------------ the child: one tree, one setting
def _rows(root):
    sys.path.insert(0, root)
    import ctypes as C

    from panfusion_amd import _lib
    lib = _lib.lib()
    has_plan = hasattr(lib, "pf_groupnorm_plan")
    fields = lambda g, names: [getattr(g, f) for f in names]
    out = dict(gn=[], bwd=[], ln=[])
    for p in gn_problems():
        # (the query divides by the pixels per chunk: 0 where there is no pixel -- asked only where its own arguments are positive)
        row = [lib.pf_groupnorm_workspace_size(p["n"], p["hw"], p["c0"] + p["c1"]) if p["n"] > 0 and p["hw"] > 0 else 0]
        if has_plan:
            g = _lib.GnPlan()
            row += [lib.pf_groupnorm_plan(p["n"], p["hw"], p["c0"], p["c1"], p["groups"], p["dtype"], p["rows0"], p["rows1"], C.byref(g))]
            row += fields(g, GN_FIELDS)
        out["gn"].append(row + [-1] * (len(GN_COLUMNS) - len(row)))
    for p in bwd_problems():
        Cc = p["c0"] + p["c1"]
        row = [lib.pf_groupnorm_bwd_workspace_size(p["n"], p["hw"], p["groups"]), lib.pf_groupnorm_param_grads_workspace_size(p["n"], p["hw"], Cc)]
        if has_plan:
            g = _lib.GnBwdPlan()
            row += [lib.pf_groupnorm_bwd_plan(p["n"], p["hw"], p["c0"], p["c1"], p["groups"], C.byref(g))] + fields(g, BWD_FIELDS)
        out["bwd"].append(row + [-1] * (len(BWD_COLUMNS) - len(row)))
    for p in ln_problems():
        row = [lib.pf_layernorm_bwd_parts(p["rows"])]
        if has_plan:
            g = _lib.LnPlan()
            row += [lib.pf_layernorm_plan(p["rows"], p["C"], C.byref(g))] + fields(g, LN_FIELDS)
        out["ln"].append(row + [-1] * (len(LN_COLUMNS) - len(row)))
    return out


def tables(root=ROOT):
    """{kind: int64 [len(ENVS), problems of the kind, columns of the kind]} of the tree at `root` and the library built in it (the plan
    columns -1 for a library without the planner)."""
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
    return {kind: np.array([o[kind] for o in out], dtype=np.int64) for kind in ("gn", "bwd", "ln")}


if __name__ == "__main__":
    print(json.dumps(_rows(sys.argv[1])))
