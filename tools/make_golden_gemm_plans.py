"""tests/golden/gemm_plans.npz: what the library named by PF_HIP_LIB plans for the fixed grid of pf_conv_gemm problems in
tests/gemm_plan_grid.py -- per problem the three queries (pf_conv_gemm_workspace_size / _gn_rows / _kernel_id) and the whole
pf_conv_plan with and without GroupNorm moments, under the default knobs, PF_GEMM32=1 and PF_GN_EPILOGUE_RES=1.
tests/test_gemm_plans.py requires the current library to reproduce it row for row.  Prints the smallest problem of every plan
class (the cases of tests/test_gpu_kernels.py::test_conv_gemm_plan_classes).  No GPU needed:

    PF_HIP_LIB=/path/to/libpanfusion_hip.so python tools/make_golden_gemm_plans.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gemm_plan_grid as G  # noqa: E402
from panfusion_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gemm_plans.npz")


def main():
    lib = _lib.lib()
    tab = G.table(lib)
    assert tab.min() >= -1 and tab[:, :, 1:].max() < 2 ** 31
    best = G.smallest_members(tab)
    missing = [c for c in G.CLASSES if c not in best]
    for c, (macs, e, p, wm) in sorted(best.items(), key=lambda kv: kv[1][0]):
        print("%-22s %8.1f MMAC  env %-24s moments %d  %s" % (c, macs / 1e6, G.ENVS[e] or "default", wm, p))
    assert not missing, "the grid has no member of plan classes %s" % missing
    # (workspace_size and the two workspace_bytes columns need 64 bits; everything else is small)
    np.savez_compressed(OUT, columns=np.array(G.COLUMNS), envs=np.array([repr(e) for e in G.ENVS]),
                        wide=tab[:, :, [0, G.COLUMNS.index("p0_workspace_bytes"), G.COLUMNS.index("p1_workspace_bytes")]],
                        table=tab.astype(np.int32))
    print("wrote %s: %d problems x %d settings, %d bytes, library %s" % (OUT, tab.shape[1], tab.shape[0], os.path.getsize(OUT), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
