"""tests/golden/linear_ws_plans.npz: routes and plans of the fixed grid of pf_linear_ws problems in tests/linear_ws_plan_grid.py, under
every setting of the seven knobs.  tests/test_linear_ws_plans.py requires the current tree to reproduce it row for row.  Two arrays,
written by two runs (each keeps the other's array).  No GPU needed:

    python tools/make_golden_linear_ws_plans.py --parent /path/to/older/checkout
        parent: the columns `route` and `supported_query` of a built checkout from BEFORE pf_linear_ws_plan existed (a git worktree
        outside this repository; the grid's harness touches only names that tree has too)
    python tools/make_golden_linear_ws_plans.py
        table: routes, the query and the whole pf_lws_plan of this tree.  Refused unless the grid columns of every supported row equal
        what the older pf_linear_ws derived for itself (parent_grid below) and every launch class has a member.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import linear_ws_plan_grid as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "linear_ws_plans.npz")


def parent_grid(M, N, K, mode):
    """TRANSCRIPTION of pf_linear_ws.hip:524-530 as it was before the planner (the launch's own derivation of channels per workgroup and
    grid split, for a problem pf_linear_ws_supported accepted) -> (chb, nblocks, splits_per_xcd, flat_splits, ntiles).  Kept word for
    word; not shared with anything the library or the tests compute."""
    k640, k1280 = K == 640, K == 1280
    chb128 = k640 and (mode == G.VT or not (N % 256 == 0 and (mode == G.L16 or mode == G.GEGLU)))
    chb = 128 if (chb128 or k1280) else 256 if k640 else 320
    nblocks = N // chb
    splits_per_xcd = 32 // nblocks
    flat_splits = 0 if 8 * splits_per_xcd * nblocks >= 200 else max(1, 256 // nblocks)
    ntiles = -(-M // (16 if k1280 else 32 if k640 else 64))
    return chb, nblocks, splits_per_xcd, flat_splits, ntiles


def main():
    keep = dict(np.load(OUT)) if os.path.exists(OUT) else {}
    probs = G.problems()
    if "--parent" in sys.argv[1:]:
        tab = G.table(os.path.abspath(sys.argv[sys.argv.index("--parent") + 1]))
        assert (tab[:, :, 2:] == -1).all(), "that checkout already has pf_linear_ws_plan"
        keep["parent"] = tab[:, :, :2]
    else:
        tab = G.table()
        col = lambda name: tab[:, :, G.COLUMNS.index(name)]
        for e in range(len(G.ENVS)):
            for i, p in enumerate(probs):
                if not col("supported")[e, i]:
                    continue
                chb, nblocks, per_xcd, flat, ntiles = parent_grid(p["M"], p["N"], p["K"], p["mode"])
                # (the older launch handed the kernel a splits_per_xcd it ignores when flat_splits > 0; the plan reports 0 there)
                want = (chb, nblocks, 0 if flat else per_xcd, flat, ntiles)
                got = tuple(int(col(f)[e, i]) for f in ("chb", "nblocks", "splits_per_xcd", "flat_splits", "ntiles"))
                assert got == want, "setting %s, problem %s: the plan says %s, the older launch derived %s" % (G.ENVS[e], p, got, want)
        seen = {G.plan_class(p, dict(zip(G.COLUMNS, tab[e, i]))) for e in range(len(G.ENVS)) for i, p in enumerate(probs) if col("supported")[e, i]}
        missing = [c for c in G.CLASSES if c not in seen]
        assert not missing, "the grid has no member of launch classes %s" % missing
        keep["table"] = tab
    keep.update(columns=np.array(G.COLUMNS), envs=np.array([repr(e) for e in G.ENVS]), problems=np.array([repr(p) for p in probs]))
    np.savez_compressed(OUT, **keep)
    print("wrote %s (%s): %d problems x %d settings, %d bytes" % (OUT, ", ".join(sorted(keep)), tab.shape[1], tab.shape[0], os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
