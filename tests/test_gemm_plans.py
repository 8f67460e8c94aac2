"""pf_conv_gemm plans one problem in one place: pf_conv_gemm_plan, of which the three older queries are projections and which the
launch itself resolves.  The plans of a fixed grid of problems (tests/gemm_plan_grid.py) must equal tests/golden/gemm_plans.npz --
written by tools/make_golden_gemm_plans.py from the planning code as it was before the planner existed -- row for row, under the
default knobs, PF_GEMM32=1 and PF_GN_EPILOGUE_RES=1.  Host arithmetic on fake pointers: no GPU."""
import ctypes as C
import functools
import os

import numpy as np

import gemm_plan_grid as G
from conftest import GOLDEN
from panfusion_amd import _lib
from test_abi import _conv_desc


@functools.lru_cache(maxsize=1)
def current_table():
    tab = G.table(_lib.lib())
    tab.setflags(write=False)
    return tab


def col(tab, name):
    return tab[:, :, G.COLUMNS.index(name)]


def test_plans_equal_the_fixture_row_for_row():
    fx = np.load(os.path.join(GOLDEN, "gemm_plans.npz"))
    assert tuple(fx["columns"]) == G.COLUMNS and tuple(fx["envs"]) == tuple(repr(e) for e in G.ENVS)
    want = fx["table"].astype(np.int64)
    wide = [0, G.COLUMNS.index("p0_workspace_bytes"), G.COLUMNS.index("p1_workspace_bytes")]
    want[:, :, wide] = fx["wide"]
    tab = current_table()
    assert tab.shape == want.shape
    bad = np.argwhere((tab != want).any(axis=2))
    probs = G.problems()
    assert len(bad) == 0, "%d rows differ; first: setting %s, problem %s: got %s, fixture %s" % (
        len(bad), G.ENVS[bad[0][0]], probs[bad[0][1]], dict(zip(G.COLUMNS, tab[tuple(bad[0])])), dict(zip(G.COLUMNS, want[tuple(bad[0])])))


def test_queries_are_projections_of_the_plan_and_plans_are_consistent():
    tab = current_table()
    ws0, ws1 = col(tab, "p0_workspace_bytes"), col(tab, "p1_workspace_bytes")
    assert (col(tab, "kernel_id") == col(tab, "p0_kernel")).all()
    assert (col(tab, "gn_rows_query") == col(tab, "p1_gn_rows")).all()
    assert (col(tab, "p0_gn_rows") == 0).all()
    # workspace_size: room for the launch with and the launch without moments (a moment launch that fails -- a residual whose plan
    # cannot emit them -- does not count); never less than either plan that can run
    has_res = np.array([bool(p.get("res")) for p in G.problems()])[None, :]
    counts1 = ~(has_res & (col(tab, "p1_gn_rows") == 0))
    assert (col(tab, "workspace_size") == np.maximum(ws0, np.where(counts1, ws1, 0))).all()
    assert (ws0 <= col(tab, "workspace_size")).all() and (np.where(col(tab, "p1_gn_rows") > 0, ws1, 0) <= col(tab, "workspace_size")).all()
    # moments: never from a split plan, and images are whole runs
    rows_per_img = np.array([(d.h_out * d.w_out) // (4 if d.subpixel else 1) for d in (G.descriptor(**p) for p in G.problems())])[None, :]
    r = col(tab, "p1_gn_rows")
    on = r > 0
    assert on.any() and (col(tab, "p1_splits")[on] == 1).all() and (col(tab, "p1_m_split")[on] == 0).all()
    assert (np.broadcast_to(rows_per_img, r.shape)[on] % r[on] == 0).all()
    for w in ("p0_", "p1_"):
        split = (col(tab, w + "splits") > 1) | (col(tab, w + "m_split") > 0)
        assert ((col(tab, w + "workspace_bytes") > 0) == split).all()
        assert ((col(tab, w + "n_tickets") > 0) == (split & (col(tab, w + "kernel") != 2))).all()


def test_every_plan_class_has_a_member():
    best = G.smallest_members(current_table())
    assert sorted(c for c in G.CLASSES if c not in best) == []


def test_moment_launch_states_the_rows_its_buffer_was_sized_for():
    """pf_conv_desc.gn_rows: a launch with gn_partial whose plan resolves to another R than the caller sized the buffer for (a plan
    cached under other PF_GEMM32 / PF_GN_EPILOGUE_RES settings) fails before anything is launched, naming both numbers."""
    lib = _lib.lib()
    kw = dict(n_out=128, out_ld=128, gn_partial=0x80000)
    g = G.plan(lib, _conv_desc(**kw), 1)
    assert g.gn_rows == 32 and g.kernel == 0
    for stated in (0, 16, 64):
        assert lib.pf_conv_gemm(C.byref(_conv_desc(gn_rows=stated, **kw)), None) == 1
        msg = lib.pf_last_error_string()
        assert b"gn_rows = %d " % stated in msg and b"runs of 32 rows" in msg, msg
    # a problem that cannot emit moments at all (GEGLU) keeps its own message, whatever gn_rows says
    d = _conv_desc(gn_rows=32, epilogue=1, **kw)
    assert lib.pf_conv_gemm_gn_rows(C.byref(d)) == 0
    assert lib.pf_conv_gemm(C.byref(d), None) == 1 and b"cannot emit GroupNorm moments" in lib.pf_last_error_string()
