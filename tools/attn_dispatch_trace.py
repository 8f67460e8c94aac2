"""Which kernels pf_attention and pf_attention_bwd launch for the problems of tests/attention_plan_grid.py and
tests/attn_bwd_plan_grid.py -- the check that a library's plans (pf_attention_plan, pf_attention_bwd_plan) ARE its launches, and that
two builds of the library launch the same kernels.

On the GPU, once per setting of the PF_ATTENTION_* / PF_ATTN_BWD_* knobs and per library (PF_HIP_LIB selects another build; one from
before either planner existed works too), under the profiler's kernel trace:

    PF_ATTENTION_OCC32=5 rocprofv3 --kernel-trace --output-format csv -d out/occ32_5 -- python tools/attn_dispatch_trace.py run out/occ32_5/plans.json

launches every problem of the grid once on seeded operands and writes what the library planned for each (null for a library without
the planner).  On the CPU, from the files that came back:

    python tools/attn_dispatch_trace.py compare out/new out/parent

walks the setting directories of both trees: per problem the sequence of (kernel name with template arguments, grid, workgroup size,
LDS bytes) must be identical between the two, and equal what the first tree's plans say (forward: the kernel and its k_attention_merge;
backward: the dq and dkv kernels and k_attn_bwd_reduce)."""
import csv
import ctypes as C
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_plan_grid as G  # noqa: E402
import attn_bwd_plan_grid as GB  # noqa: E402


def run(out_json):
    import torch

    from panfusion_amd import _lib
    lib = G.load()
    lib.pf_attention.restype, lib.pf_attention.argtypes = _lib.SIGNATURES["pf_attention"]
    dev, dtype = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(7)
    planned = []
    for p in G.problems():
        d = G.descriptor(**p)
        C_ = p["H"] * p["D"]
        qk = torch.randn(p["B"] * max(p["nq"], p["nk"] + 64) * d.q_ld, device=dev, generator=gen).mul_(0.5).to(dtype)
        k = qk if p["wide"] == 2 else torch.randn(p["B"] * (p["nk"] + 64) * d.k_ld, device=dev, generator=gen).mul_(0.5).to(dtype)
        vt = torch.randn(p["B"] * C_ * d.vt_ld, device=dev, generator=gen).to(dtype)
        out = torch.empty(p["B"] * p["nq"] * d.o_ld, device=dev, dtype=dtype)
        d.q, d.k, d.vt, d.out = qk.data_ptr(), k.data_ptr() + (2 * C_ if p["wide"] == 2 else 0), vt.data_ptr(), out.data_ptr()
        d.q_bs = max(p["nq"], p["nk"] + 64) * d.q_ld if p["wide"] == 2 else p["nq"] * d.q_ld
        d.k_bs = d.q_bs if p["wide"] == 2 else (p["nk"] + 64) * d.k_ld
        keep = [qk, k, vt, out]
        if p["bias"]:                                              # no tile flagged: the table is never read, the dispatch is the same
            keep += [torch.zeros(p["nq"], p["nk"], device=dev), torch.zeros((p["nq"] + 31) // 32, (p["nk"] + 31) // 32, dtype=torch.uint8, device=dev)]
            d.bias, d.flags = keep[-2].data_ptr(), keep[-1].data_ptr()
        if p["lse"]:
            keep.append(torch.empty(p["B"] * p["H"] * p["nq"], device=dev))
            d.lse = keep[-1].data_ptr()
        nbytes = lib.pf_attention_workspace_size(C.byref(d))
        if nbytes:
            keep.append(torch.empty(nbytes, dtype=torch.uint8, device=dev))
            d.workspace, d.workspace_bytes = keep[-1].data_ptr(), nbytes
        planned.append({f: getattr(G.plan(lib, d), f) for f in G.PLAN_FIELDS} if lib.has_plan else None)
        status = lib.pf_attention(C.byref(d), None)
        torch.cuda.synchronize()
        assert status == 0 and bool(torch.isfinite(out.view(p["B"], p["nq"], d.o_ld)[:, :, :C_].float()).all()), (p, status)
    bwd_planned = run_backward(gen)
    with open(out_json, "w") as fh:
        json.dump(dict(library=_lib.LIB_PATH, problems=[repr(p) for p in G.problems()], plans=planned,
                       bwd_problems=[repr(p) for p in GB.problems()], bwd_plans=bwd_planned), fh)
    print("launched %d forward and %d backward problems on %s" % (len(planned), len(bwd_planned), _lib.LIB_PATH))


def run_backward(gen):
    """Every problem of the backward grid once: operands of the descriptor's sizes (the transposes need not be transposes for the
    dispatch), an lse large enough that every probability is tiny.  Returns the plans (None for a library without the planner)."""
    import torch

    from panfusion_amd import _lib
    lib = GB.load()
    lib.pf_attention_bwd.restype, lib.pf_attention_bwd.argtypes = _lib.SIGNATURES["pf_attention_bwd"]
    dev, dtype = "cuda", torch.bfloat16
    planned = []
    for p in GB.problems():
        d = GB.descriptor(**p)
        B, Cc = p["B"], p["H"] * p["D"]
        rnd = lambda n: torch.randn(n, device=dev, generator=gen).mul_(0.5).to(dtype)
        keep = dict(q=rnd(B * d.q_bs), k=rnd(B * d.k_bs), v=rnd(B * d.v_bs), dout=rnd(B * d.do_bs), qt=rnd(B * d.qt_bs), kt=rnd(B * d.kt_bs),
                    dot=rnd(B * d.dot_bs), dq=torch.zeros(B * d.dq_bs, device=dev, dtype=dtype), dk=torch.zeros(B * d.dk_bs, device=dev, dtype=dtype),
                    dv=torch.zeros(B * d.dv_bs, device=dev, dtype=dtype), lse=torch.full((B * p["H"] * p["nq"],), 40.0, device=dev),
                    delta=torch.zeros(B * p["H"] * p["nq"], device=dev))
        for f, t in keep.items():
            setattr(d, f, t.data_ptr())
        if p["bias"]:                                              # no tile flagged: the table is never read, the dispatch is the same
            keep["bias"] = torch.zeros(p["nq"], p["nk"], device=dev)
            keep["flags"] = torch.zeros((p["nq"] + 31) // 32, (p["nk"] + 31) // 32, dtype=torch.uint8, device=dev)
            d.bias, d.flags = keep["bias"].data_ptr(), keep["flags"].data_ptr()
        nbytes = lib.pf_attention_bwd_workspace_size(C.byref(d))
        if nbytes:
            keep["ws"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            d.workspace, d.workspace_bytes = keep["ws"].data_ptr(), nbytes
        planned.append({f: getattr(GB.plan(lib, d), f) for f in GB.PLAN_FIELDS} if lib.has_plan else None)
        status = lib.pf_attention_bwd(C.byref(d), None)
        torch.cuda.synchronize()
        assert status == 0 and all(bool(torch.isfinite(keep[f].float()).all()) for f in ("dq", "dk", "dv")), (p, status)
    return planned


def launches(setting_dir, family="k_attention", follower="k_attention_merge"):
    """Per problem the kernels of one family in launch order: [(name, grid xyz in workgroups, workgroup size, LDS bytes)].  A kernel whose
    name contains one of `follower` belongs to the problem of the launch before it."""
    files = glob.glob(os.path.join(setting_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (setting_dir, files)
    rows = [r for r in csv.DictReader(open(files[0])) if family in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        item = (re.sub(r"\s+", " ", r["Kernel_Name"]), tuple(int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg)), wg[0], int(r["LDS_Block_Size"]))
        if any(f in item[0] for f in follower.split("|")):
            out[-1].append(item)
        else:
            out.append([item])
    return out


def expected(p, g):
    """What plan g of problem p says the trace shows: (kernel name fragments, grid, threads) and whether a merge launch follows."""
    if g["kernel"] == 1:
        frag = "k_attention_lds<%s, %d, %s, %s, %d, %s>" % ("pf::Bf16", p["D"], str(bool(p["bias"])).lower(), str(bool(g["pipelined"])).lower(),
                                                           g["occupancy"], str(bool(g["msum"])).lower())
    else:
        frag = {0: "k_attention<pf::Bf16, %d>" % p["D"], 2: "k_attention_pp<pf::Bf16>", 3: "k_attention_pp2<pf::Bf16>"}[g["kernel"]]
    return frag, (g["grid_x"], g["grid_y"], g["grid_z"]), g["threads"], g["splits"] > 1


def expected_bwd(p, g):
    """What plan g of backward problem p says the trace shows: [(kernel name fragment, grid, threads)] in launch order."""
    args = {0: "<pf::Bf16, %d, false>", 1: "<pf::Bf16, %d, true>", 2: "_lds<pf::Bf16, %d>"}[g["kernel"]] % p["D"]
    out = [("k_attn_bwd_dq" + args, tuple(g["dq_grid_" + a] for a in "xyz"), g["threads"]),
           ("k_attn_bwd_dkv" + args, tuple(g["dkv_grid_" + a] for a in "xyz"), g["threads"])]
    if g["qsplit"] > 1:
        out.append(("k_attn_bwd_reduce<pf::Bf16>", tuple(g["reduce_grid_" + a] for a in "xyz"), 256))
    return out


def compare_bwd(s, meta, new_root, parent_root):
    probs = [eval(p) for p in meta["bwd_problems"]]
    new, par = (launches(os.path.join(r, s), "k_attn_bwd", "k_attn_bwd_dkv|k_attn_bwd_reduce") for r in (new_root, parent_root))
    assert len(new) == len(par) == len(probs), (s, len(new), len(par), len(probs))
    n_bad = 0
    for p, g, a, b in zip(probs, meta["bwd_plans"], new, par):
        want = expected_bwd(p, g)
        ok = a == b and len(a) == len(want) and all(w[0] in x[0].replace("(pf::AttnBwdParams)", "") and x[1] == w[1] and x[2] == w[2] for x, w in zip(a, want))
        if not ok:
            n_bad += 1
            print("MISMATCH %s %s\n  plan   %s\n  new    %s\n  parent %s" % (s, p, g, a, b))
    print("%-40s %3d backward problems, %3d launches, %d mismatches" % (s, len(probs), sum(len(a) for a in new), n_bad))
    return n_bad


def compare(new_root, parent_root):
    bad = 0
    settings = sorted(os.path.basename(d) for d in glob.glob(os.path.join(new_root, "*")) if os.path.isdir(d))
    for s in settings:
        meta = json.load(open(os.path.join(new_root, s, "plans.json")))
        probs = [eval(p) for p in meta["problems"]]
        new, par = launches(os.path.join(new_root, s)), launches(os.path.join(parent_root, s))
        assert len(new) == len(par) == len(probs), (s, len(new), len(par), len(probs))
        n_bad = 0
        for p, g, a, b in zip(probs, meta["plans"], new, par):
            frag, grid, threads, merge = expected(p, g)
            ok = a == b and frag in a[0][0].replace("(pf::AttnParams)", "") and a[0][1] == grid and a[0][2] == threads and (len(a) == 2) == merge
            if not ok:
                n_bad += 1
                print("MISMATCH %s %s\n  plan   %s\n  new    %s\n  parent %s" % (s, p, g, a, b))
        print("%-40s %3d problems, %3d launches, %d mismatches" % (s, len(probs), sum(len(a) for a in new), n_bad))
        bad += n_bad + compare_bwd(s, meta, new_root, parent_root)
    print("settings: %d, mismatches: %d" % (len(settings), bad))
    return 1 if bad or not settings else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(sys.argv[2], sys.argv[3]))
