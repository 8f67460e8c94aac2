"""tests/golden/norm_plans.npz: queries and plans of the fixed grid of GroupNorm / LayerNorm problems in tests/norm_plan_grid.py, under both
settings of PF_GN_DIRECT_MAX.  tests/test_norm_plans.py requires the current tree to reproduce it row for row.  Per table (gn, bwd, ln) two
arrays, written by two runs (each keeps the other's arrays).  No GPU needed:

    python tools/make_golden_norm_plans.py --parent /path/to/older/checkout
        *_parent: the size queries (pf_groupnorm_workspace_size, pf_groupnorm_bwd_workspace_size, pf_groupnorm_param_grads_workspace_size,
        pf_layernorm_bwd_parts) of a built checkout from BEFORE the planner existed (a git worktree outside this repository; the grid's
        harness touches only names that tree has too)
    python tools/make_golden_norm_plans.py
        *_table: the queries, the planners' status and the whole plans of this tree.  Refused unless every class of launch decision
        (norm_plan_grid.CLASSES) has a member.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import norm_plan_grid as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "norm_plans.npz")


def main():
    keep = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    if "--parent" in sys.argv[1:]:
        tabs = G.tables(os.path.abspath(sys.argv[sys.argv.index("--parent") + 1]))
        for kind, tab in tabs.items():
            assert (tab[:, :, G.N_PARENT[kind]:] == -1).all(), "that checkout already has the planner"
            keep[kind + "_parent"] = tab[:, :, :G.N_PARENT[kind]]
    else:
        tabs = G.tables()
        missing = G.missing_classes(tabs)
        assert not missing, "the grid has no member of %s" % missing
        for kind, tab in tabs.items():
            keep[kind + "_table"] = tab
    keep["envs"] = np.array([repr(e) for e in G.ENVS])
    for kind in tabs:
        keep[kind + "_columns"] = np.array(G.COLUMNS[kind])
        keep[kind + "_problems"] = np.array([repr(p) for p in G.PROBLEMS[kind]()])
    np.savez_compressed(OUT, **keep)
    print("wrote %s (%s): %s problems x %d settings, %d bytes" % (OUT, ", ".join(sorted(keep)), [t.shape[1] for t in tabs.values()],
                                                                 len(G.ENVS), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
