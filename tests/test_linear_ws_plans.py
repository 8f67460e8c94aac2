"""pf_linear_ws plans one problem in one place: pf_linear_ws_plan, of which pf_linear_ws_supported is a projection, which the launch
resolves and which the linear front ends of ops.py ask for their routing.  For a fixed grid of problems (tests/linear_ws_plan_grid.py)
under every setting of the seven knobs, routes and plans must equal tests/golden/linear_ws_plans.npz row for row; the fixture's `parent`
columns (route, pf_linear_ws_supported) came from the tree as it was before the planner existed, when the routing rule was Python in
ops.py (tools/make_golden_linear_ws_plans.py).  Host arithmetic on tensors without storage: no GPU."""
import ctypes as C
import functools
import os

import numpy as np

import linear_ws_plan_grid as G
from conftest import GOLDEN
from panfusion_amd import _lib


@functools.lru_cache(maxsize=1)
def current_table():
    tab = G.table()
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=1)
def fixture():
    fx = np.load(os.path.join(GOLDEN, "linear_ws_plans.npz"))
    assert tuple(fx["columns"]) == G.COLUMNS and tuple(fx["envs"]) == tuple(repr(e) for e in G.ENVS)
    assert tuple(fx["problems"]) == tuple(repr(p) for p in G.problems())
    return fx


def col(tab, name):
    return tab[:, :, G.COLUMNS.index(name)]


def per_problem(f, like):
    return np.broadcast_to(np.array([f(p) for p in G.problems()])[None, :], like.shape)


def describe(tab, want, bad):
    e, i = bad[0]
    return "%d rows differ; first: setting %s, problem %s: got %s, want %s" % (len(bad), G.ENVS[e], G.problems()[i], tab[e, i], want[e, i])


def test_routes_and_support_equal_the_parents_row_for_row():
    tab, parent = current_table(), fixture()["parent"]
    got = tab[:, :, :2]
    assert got.shape == parent.shape
    bad = np.argwhere((got != parent).any(axis=2))
    assert len(bad) == 0, describe(got, parent, bad)
    assert (col(tab, "supported") == col(tab, "supported_query")).all()          # the query is a projection of the plan
    # every setting moves some route, except PF_LWS_COUNTED, which moves none
    for e, env in enumerate(G.ENVS[1:], 1):
        assert (got[e, :, 0] != got[0, :, 0]).any() == ("PF_LWS_COUNTED" not in env), env


def test_preferred_is_the_route_to_linear_ws():
    tab = current_table()
    mode = per_problem(lambda p: p["mode"], col(tab, "route"))
    assert ((col(tab, "preferred") == 1) == (col(tab, "route") == G.ROUTE_WS + mode)).all()
    assert (col(tab, "preferred") <= col(tab, "supported")).all() and set(np.unique(col(tab, "preferred"))) == {0, 1}


def test_plans_equal_the_fixture_row_for_row():
    tab, want = current_table(), fixture()["table"]
    assert tab.shape == want.shape
    bad = np.argwhere((tab != want).any(axis=2))
    assert len(bad) == 0, describe(tab, want, bad)


def test_plans_are_consistent():
    tab = current_table()
    on = col(tab, "supported") == 1
    assert on.any() and (~on).any() and (tab[~on][:, 2:] == 0).all()               # an unsupported problem has an all-zero plan
    M, N, K = (per_problem(lambda p, f=f: p[f], on) for f in ("M", "N", "K"))
    k, chb, tile, nblocks, ntiles = (col(tab, f) for f in ("k", "chb", "tile_tokens", "nblocks", "ntiles"))
    assert (k[on] == K[on]).all() and (tile[on] * k[on] == 64 * 320).all()         # a ring slot is 40 KB at every K
    assert ((nblocks * chb)[on] == N[on]).all() and (ntiles[on] == -(-M[on] // tile[on])).all()
    assert np.isin(chb[on], (320, 256, 128)).all() and (M[on] >= tile[on]).all()
    grouped, flat = col(tab, "splits_per_xcd"), col(tab, "flat_splits")
    assert ((grouped[on] > 0) != (flat[on] > 0)).all() and (grouped[on] > 0).any() and (flat[on] > 0).any()
    g = on & (grouped > 0)
    assert (8 * grouped * nblocks)[g].max() <= 256 and (8 * grouped * nblocks)[g].min() >= 200
    f = on & (flat > 0)
    assert ((flat * nblocks)[f & (nblocks <= 256)] <= 256).all() and (8 * (32 // nblocks[f]) * nblocks[f]).max() < 200
    counted = np.array(["PF_LWS_COUNTED" not in e for e in G.ENVS])[:, None]
    assert (col(tab, "counted")[on] == np.broadcast_to(counted, on.shape)[on]).all()
    # nothing but `preferred`, `counted` and the route depends on a knob
    shape_cols = [G.COLUMNS.index(c) for c in G.COLUMNS if c not in ("route", "preferred", "counted")]
    assert (tab[:, :, shape_cols] == tab[:1, :, shape_cols]).all()


def test_every_launch_class_and_layout_has_a_member():
    tab, P = current_table(), G.problems()
    rows = [(p, dict(zip(G.COLUMNS, tab[0, i]))) for i, p in enumerate(P) if tab[0, i, G.COLUMNS.index("supported")]]
    seen = {G.plan_class(p, g) for p, g in rows}
    assert sorted(c for c in G.CLASSES if c not in seen) == [] and sorted(c for c in seen if c not in G.CLASSES) == []
    assert len(G.CLASSES) == 13
    for k in (320, 640, 1280):                                                    # both grid layouts at every K
        assert {g["flat_splits"] > 0 for p, g in rows if g["k"] == k} == {False, True}, k


def test_the_plan_reads_no_pointer_and_null_arguments_have_no_plan():
    lib = _lib.lib()
    plans = []
    for ptr in (None, 0x10000):
        d, g = _lib.LinearWsDesc(), _lib.LwsPlan()
        d.M, d.N, d.K, d.mode, d.a_ld, d.dtype, d.rows_per_batch = 163840, 960, 320, G.QKV, 320, _lib.PF_BF16, 4096
        d.a = d.w = d.bias = d.residual = d.out = d.out_vt = d.ln_gamma = d.ln_beta = d.ln_out = ptr
        assert lib.pf_linear_ws_plan(C.byref(d), C.byref(g)) == 0
        plans.append(bytes(g))
        assert g.supported == 1 and g.preferred == 1 and (g.k, g.chb, g.tile_tokens, g.nblocks) == (320, 320, 64, 3)
    assert plans[0] == plans[1]
    assert lib.pf_linear_ws_plan(None, C.byref(g)) == 1 and b"pf_linear_ws_plan" in lib.pf_last_error_string()
    assert lib.pf_linear_ws_plan(C.byref(d), None) == 1
    d.mode = 7                                                                    # out of range: no plan, no support, refused before the shape is looked at
    assert lib.pf_linear_ws_plan(C.byref(d), C.byref(g)) == 0 and bytes(g) == bytes(_lib.LwsPlan())
    assert lib.pf_linear_ws_supported(163840, 960, 320, 7) == 0
    assert lib.pf_linear_ws(C.byref(d), None) == 1 and b"unknown mode 7" in lib.pf_last_error_string()
