"""tests/golden/attn_bwd_plans.npz: what the library plans for the fixed grid of pf_attention_bwd problems in
tests/attn_bwd_plan_grid.py, under every PF_ATTN_BWD_* setting of that grid.  tests/test_attn_bwd_plans.py requires the current
library to reproduce it row for row.  Two arrays, written by two runs (each keeps the other's array).  No GPU needed:

    PF_HIP_LIB=/path/to/older/libpanfusion_hip.so python tools/make_golden_attn_bwd_plans.py --parent-workspace
        parent_workspace_size: pf_attention_bwd_workspace_size of a library from BEFORE pf_attention_bwd_plan existed (it exports that
        query); the scratch size is a function of the query split, so this column pins qsplit on every row
    python tools/make_golden_attn_bwd_plans.py
        table: the query and the whole pf_attn_bwd_plan from the in-tree library (tools/attn_dispatch_trace.py compares these plans with
        the kernels a library launches)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attn_bwd_plan_grid as G  # noqa: E402
from panfusion_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "attn_bwd_plans.npz")


def main():
    keep = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    tab = G.table()
    probs = G.problems()
    if "--parent-workspace" in sys.argv[1:]:
        keep["parent_workspace_size"] = tab[:, :, 0]
    else:
        seen = {G.plan_class(p, dict(zip(G.PLAN_FIELDS, tab[e, i, 1:]))) for e in range(len(G.ENVS)) for i, p in enumerate(probs)}
        missing = [c for c in G.CLASSES if c not in seen]
        assert not missing, "the grid has no member of launch classes %s" % missing
        keep["table"] = tab
    keep.update(columns=np.array(G.COLUMNS), envs=np.array([repr(e) for e in G.ENVS]), problems=np.array([repr(p) for p in probs]))
    np.savez_compressed(OUT, **keep)
    print("wrote %s (%s): %d problems x %d settings, %d bytes, library %s" % (OUT, ", ".join(sorted(keep)), tab.shape[1], tab.shape[0],
                                                                           os.path.getsize(OUT), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
