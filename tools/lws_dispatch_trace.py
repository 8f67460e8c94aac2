"""Which kernels pf_linear_ws launches -- the check that a library's plans (pf_linear_ws_plan) ARE its launches, and that two builds of
the library launch the same kernels.  The problems: of tests/linear_ws_plan_grid.py the smallest member of every launch class (by the
committed fixture, so that both builds run the same list) and the benchmark step's launches.

On the GPU, once per setting of PF_LWS_COUNTED and per library (PF_HIP_LIB selects another build; one from before pf_linear_ws_plan
existed works too), under the profiler's kernel trace and nothing else:

    rocprofv3 --kernel-trace --output-format csv -d out/new/default -- python tools/lws_dispatch_trace.py run out/new/default/plans.json

launches every problem once on seeded operands and writes what the library planned for each (null for a library without the planner).
On the CPU, from the files that came back:

    python tools/lws_dispatch_trace.py compare out/new out/parent

walks the setting directories of both trees: per problem the kernel name (it carries T, MODE, COUNTED, K and CHB), grid and workgroup
size must be identical between the two, and equal what the first tree's plan says."""
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


def problems():
    import numpy as np

    import linear_ws_plan_grid as G
    fx = np.load(os.path.join(ROOT, "tests", "golden", "linear_ws_plans.npz"))
    P, tab = G.problems(), fx["table"][0]
    assert tuple(fx["problems"]) == tuple(repr(p) for p in P)
    ok = lambda i: tab[i, G.COLUMNS.index("supported")] and P[i]["a_ld"] % 8 == 0 and P[i]["dtype"] == "bf16" and \
        (G.rows_per_batch(P[i]) == 0 or (P[i]["M"] % P[i]["n_batch"] == 0 and G.rows_per_batch(P[i]) % tab[i, G.COLUMNS.index("tile_tokens")] == 0))
    out = []
    for c in G.CLASSES:
        members = [i for i in range(len(P)) if ok(i) and G.plan_class(P[i], dict(zip(G.COLUMNS, tab[i]))) == c]
        out.append(P[min(members, key=lambda i: P[i]["M"] * P[i]["N"])])
    return out + [p for p in P if p["tag"] == "step"]


def run(out_json):
    import torch

    import linear_ws_plan_grid as G
    from panfusion_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)                     # (bound directly: a library from before pf_linear_ws_plan loads too)
    lib.pf_linear_ws.restype, lib.pf_linear_ws.argtypes = _lib.SIGNATURES["pf_linear_ws"]
    has_plan = hasattr(lib, "pf_linear_ws_plan")
    dev, dtype = "cuda", torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(7)
    planned = []
    for p in problems():
        M, N, K, mode, rpb = p["M"], p["N"], p["K"], p["mode"], G.rows_per_batch(p)
        x = torch.randn(M, p["a_ld"], device=dev, generator=gen).to(dtype)
        w = torch.randn(N, K, device=dev, generator=gen).mul_(K ** -0.5).to(dtype)
        n_store = N // 2 if mode == G.GEGLU else 640 if mode == G.QKV else N
        out = torch.empty(M, n_store, device=dev, dtype=torch.float32 if mode in (G.F32, G.F32_LN) else dtype)
        keep = [x, w, out]
        d = _lib.LinearWsDesc()
        d.M, d.N, d.K, d.mode, d.a_ld, d.dtype, d.rows_per_batch = M, N, K, mode, p["a_ld"], _lib.PF_BF16, rpb
        d.a, d.w, d.out, d.out_ld = x.data_ptr(), w.data_ptr(), out.data_ptr(), n_store
        if rpb:
            keep.append(torch.empty(M // rpb, 320 if mode == G.QKV else N, rpb, device=dev, dtype=dtype))
            d.out_vt, d.vt_ld, d.vt_bs = keep[-1].data_ptr(), rpb, keep[-1].stride(0)
        if mode == G.F32_LN:
            keep += [torch.ones(N, device=dev), torch.zeros(N, device=dev), torch.empty(M, N, device=dev, dtype=dtype)]
            d.ln_gamma, d.ln_beta, d.ln_out, d.ln_ld, d.ln_eps = keep[-3].data_ptr(), keep[-2].data_ptr(), keep[-1].data_ptr(), N, 1e-5
        g = None
        if has_plan:
            g = _lib.LwsPlan()
            lib.pf_linear_ws_plan.restype, lib.pf_linear_ws_plan.argtypes = _lib.SIGNATURES["pf_linear_ws_plan"]
            assert lib.pf_linear_ws_plan(C.byref(d), C.byref(g)) == 0
            g = {f: getattr(g, f) for f in G.PLAN_FIELDS}
        planned.append(g)
        status = lib.pf_linear_ws(C.byref(d), None)
        torch.cuda.synchronize()
        assert status == 0 and bool(torch.isfinite((keep[3] if mode == G.VT else out).float()).all()), (p, status)
    with open(out_json, "w") as fh:
        json.dump(dict(library=_lib.LIB_PATH, problems=[repr(p) for p in problems()], plans=planned), fh)
    print("launched %d problems on %s" % (len(planned), _lib.LIB_PATH))


def launches(setting_dir):
    """The k_linear_ws launches of the trace in launch order: (name, workgroups, workgroup size)."""
    files = glob.glob(os.path.join(setting_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (setting_dir, files)
    rows = [r for r in csv.DictReader(open(files[0])) if "k_linear_ws" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(re.sub(r"\s+", " ", r["Kernel_Name"]), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"])) for r in rows]


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
            frag = "k_linear_ws<pf::Bf16, %d, %s, %d, %d>" % (p["mode"], str(bool(g["counted"])).lower(), g["k"], g["chb"])
            if not (a == b and frag in a[0] and a[1:] == (256, 512)):
                n_bad += 1
                print("MISMATCH %s %s\n  plan   %s\n  new    %s\n  parent %s" % (s, p, g, a, b))
        print("%-20s %3d problems, %d mismatches; classes launched: %d" % (s, len(probs), n_bad, len({a[0] for a in new})))
        bad += n_bad
    print("settings: %d, mismatches: %d" % (len(settings), bad))
    return 1 if bad or not settings else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else compare(sys.argv[2], sys.argv[3]))
