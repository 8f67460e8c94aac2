"""The GroupNorm / LayerNorm launches plan one problem in one place (pf_norm_plan.hip): pf_groupnorm_plan, pf_groupnorm_bwd_plan and
pf_layernorm_plan, which the launches resolve, of which the four size queries are projections and which ops.groupnorm_scale_shift asks
for its arm.  For a fixed grid of problems (tests/norm_plan_grid.py) under both settings of PF_GN_DIRECT_MAX, queries and plans must
equal tests/golden/norm_plans.npz row for row; the fixture's `*_parent` arrays are the queries of the tree as it was before the planner
existed (tools/make_golden_norm_plans.py).  Host arithmetic on fake pointers: no GPU."""
import ctypes as C
import functools
import os

import numpy as np

import norm_plan_grid as G
from conftest import GOLDEN
from panfusion_amd import _lib

KINDS = ("gn", "bwd", "ln")


@functools.lru_cache(maxsize=1)
def current_tables():
    tabs = G.tables()
    for t in tabs.values():
        t.setflags(write=False)
    return tabs


@functools.lru_cache(maxsize=1)
def fixture():
    fx = np.load(os.path.join(GOLDEN, "norm_plans.npz"))
    assert tuple(fx["envs"]) == tuple(repr(e) for e in G.ENVS)
    for kind in KINDS:
        assert tuple(fx[kind + "_columns"]) == G.COLUMNS[kind]
        assert tuple(fx[kind + "_problems"]) == tuple(repr(p) for p in G.PROBLEMS[kind]())
    return fx


def col(kind, name, tab=None):
    return (current_tables()[kind] if tab is None else tab)[:, :, G.COLUMNS[kind].index(name)]


def describe(kind, got, want, bad):
    e, i = bad[0]
    return "%s: %d rows differ; first: setting %s, problem %s: got %s, want %s" % (kind, len(bad), G.ENVS[e], G.PROBLEMS[kind]()[i], got[e, i], want[e, i])


def test_queries_equal_the_parents_row_for_row():
    """Every row, accepted by its launch or refused: the query says what it said (the parent's queries knew no shape rule, and neither do
    these).  The one exception is the harness's: the parent's pf_groupnorm_workspace_size divided by zero without pixels, so the grid does
    not ask it there and records 0, which is what the query now answers."""
    fx = fixture()
    for kind in KINDS:
        got, parent = current_tables()[kind][:, :, :G.N_PARENT[kind]], fx[kind + "_parent"]
        assert got.shape == parent.shape
        bad = np.argwhere((got != parent).any(axis=2))
        assert len(bad) == 0, describe(kind, got, parent, bad)
        refused = col(kind, "status") != 0
        assert refused.any() and (got[refused] != 0).any()                        # refused problems with a stated size are in the grid
    lib = _lib.lib()
    assert lib.pf_groupnorm_workspace_size(1, 0, 64) == 0 and lib.pf_groupnorm_workspace_size(0, 64, 64) == 0
    # more than 512 groups: a backward the launch accepts, and a size that does not depend on the channels it is asked with
    assert lib.pf_groupnorm_bwd_workspace_size(1, 300, 1024) == (19 + 1) * 1024 * 16
    b = _lib.GnBwdPlan()
    for Cc in (1024, 4096):
        assert lib.pf_groupnorm_bwd_plan(1, 300, Cc, 0, 1024, C.byref(b)) == 0 and b.bwd_workspace_bytes == (19 + 1) * 1024 * 16


def test_queries_are_projections_of_the_plans():
    ok = col("gn", "status") == 0
    stats = ok & (col("gn", "arm") != G.FROM_PARTIALS)
    assert (col("gn", "workspace_bytes")[stats] == col("gn", "ws_query")[stats]).all()
    assert (col("gn", "workspace_bytes")[ok & ~stats] == 0).all()
    both = (col("bwd", "status") == 0) & (col("bwd", "bwd_lds_bytes") > 0)
    assert both.any() and (col("bwd", "bwd_workspace_bytes")[both] == col("bwd", "bwd_ws_query")[both]).all()
    ok = col("bwd", "status") == 0
    assert (col("bwd", "param_workspace_bytes")[ok] == col("bwd", "param_ws_query")[ok]).all()
    ok = col("ln", "status") == 0
    assert (col("ln", "bwd_parts")[ok] == col("ln", "parts_query")[ok]).all()


def test_plans_equal_the_fixture_row_for_row():
    fx = fixture()
    for kind in KINDS:
        tab, want = current_tables()[kind], fx[kind + "_table"]
        assert tab.shape == want.shape
        bad = np.argwhere((tab != want).any(axis=2))
        assert len(bad) == 0, describe(kind, tab, want, bad)


def test_every_class_of_launch_decision_has_a_member():
    assert G.missing_classes(current_tables()) == []
    assert len(G.CLASSES) == 33


def test_plans_are_consistent():
    tabs = current_tables()
    for kind in KINDS:                                                            # a refused problem has an all-zero plan
        tab = tabs[kind]
        bad = col(kind, "status") != 0
        assert set(np.unique(col(kind, "status"))) == {0, 1} and (tab[bad][:, G.N_PARENT[kind] + 1:] == 0).all()
    P, arm, ok = G.gn_problems(), col("gn", "arm"), col("gn", "status") == 0
    per = lambda f: np.broadcast_to(np.array([f(p) for p in P])[None, :], arm.shape)
    n, hw, Cc, groups = per(lambda p: p["n"]), per(lambda p: p["hw"]), per(lambda p: p["c0"] + p["c1"]), per(lambda p: p["groups"])
    assert (np.isin(arm[ok], (1, 2, 3))).all() and (arm[~ok] == 0).all()
    two, direct, part = arm == G.TWO_STAGE, arm == G.DIRECT, arm == G.FROM_PARTIALS
    ppc, nchunks, pix_par = col("gn", "ppc"), col("gn", "nchunks"), col("gn", "pix_par")
    assert (nchunks[two] == -(-hw[two] // ppc[two])).all() and (nchunks[two] <= 256).all() and (ppc[two] <= np.maximum(64, -(-hw[two] // 256))).all()
    assert (pix_par[two] == 256 // np.minimum(Cc[two] // 8, 256)).all()
    assert (col("gn", "lds_bytes")[two] == 2 * pix_par[two] * Cc[two] * 4).all() and col("gn", "lds_bytes")[two].max() == 64 * 1024
    assert (col("gn", "grid_x")[two] == nchunks[two]).all() and (col("gn", "grid_y")[two] == n[two]).all()
    assert (col("gn", "grid2_x")[two] == n[two]).all() and (col("gn", "grid2_y")[two] == -(-groups[two] // 8)).all()
    assert (col("gn", "grid_x")[direct] == n[direct]).all() and (col("gn", "grid_y")[direct] == groups[direct]).all()
    for f in ("ppc", "nchunks", "pix_par", "lds_bytes", "grid2_x", "grid2_y"):     # what an arm does not use is 0
        assert (col("gn", f)[direct | part] == 0).all(), f
    for f in ("gpb", "pairs_per_block", "slices"):
        assert (col("gn", f)[direct | two] == 0).all(), f
    gpb, ppb, slices = col("gn", "gpb"), col("gn", "pairs_per_block"), col("gn", "slices")
    assert (ppb[part] == np.minimum(gpb * (Cc // np.maximum(groups, 1)) // 2, Cc // 2)[part]).all() and ppb[part].max() == 512
    assert (slices[part] == np.where(ppb[part] <= 128, 256 // ppb[part], 1)).all()
    assert (col("gn", "grid_x")[part] == n[part]).all() and (col("gn", "grid_y")[part] == -(-groups[part] // gpb[part])).all()
    assert (col("gn", "partials_refused")[part] == 0).all()
    # PF_GN_DIRECT_MAX=0 turns every direct problem with a channel into a two-stage one (or into a refusal: the 64 KiB limit) and moves nothing else
    was = direct[0]
    assert was.any() and not direct[1].any() and (two[1] | ~ok[1])[was].all()
    assert (tabs["gn"][1][~was] == tabs["gn"][0][~was]).all()
    assert (col("gn", "workspace_bytes")[1][was & ok[1]] == col("gn", "workspace_bytes")[0][was & ok[1]]).all()
    assert (tabs["bwd"][1] == tabs["bwd"][0]).all() and (tabs["ln"][1] == tabs["ln"][0]).all()
    # backward: both partial kernels share the chunks; the members of pf_groupnorm_bwd are 0 in the plan of the parameter gradients alone
    B, okb = G.bwd_problems(), col("bwd", "status")[0] == 0
    row = lambda i: dict(zip(G.BWD_COLUMNS, tabs["bwd"][0, i]))
    for i, p in enumerate(B):
        if not okb[i]:
            continue
        g, Cb = row(i), p["c0"] + p["c1"]
        assert g["chunks"] == -(-p["hw"] // g["ppc"]) and g["ppc"] in (64, 32, 16, 8) and (g["ppc"] == 8 or g["chunks"] >= 16), p
        assert (g["partial_grid_x"], g["partial_grid_y"]) == (g["chunks"], p["n"]) and g["param_lds_bytes"] == 2 * g["pix_par"] * Cb * 4
        assert g["param_partial_bytes"] == p["n"] * g["chunks"] * 2 * Cb * 4 < g["param_workspace_bytes"]
        if p["groups"]:
            assert g["bwd_lds_bytes"] == 2 * g["param_lds_bytes"] <= 64 * 1024 and g["finalize_grid_x"] == p["n"]
            assert (g["apply_grid_x"], g["apply_grid_y"]) == (-(-p["hw"] * (Cb // 8) // 256), p["n"])
            assert g["bwd_workspace_bytes"] == p["n"] * (g["chunks"] + 1) * p["groups"] * 16
        else:
            assert [g[f] for f in ("bwd_lds_bytes", "finalize_grid_x", "apply_grid_x", "apply_grid_y", "bwd_workspace_bytes")] == [0] * 5
    L, okl = G.ln_problems(), col("ln", "status")[0] == 0
    for i, p in enumerate(L):
        if okl[i]:
            g = dict(zip(G.LN_COLUMNS, tabs["ln"][0, i]))
            assert g["grid_x"] == -(-p["rows"] // (4 * g["rows_per_wave"])) and g["bwd_parts"] == min(512, -(-p["rows"] // 4)), p


def test_the_plans_read_no_pointer():
    """The planners take scalars and the plan to fill: nothing else of theirs is a pointer, and a NULL plan is the only argument error
    that is not a refusal of the problem."""
    lib = _lib.lib()
    for name, plan in (("pf_groupnorm_plan", _lib.GnPlan), ("pf_groupnorm_bwd_plan", _lib.GnBwdPlan), ("pf_layernorm_plan", _lib.LnPlan)):
        argtypes = _lib.SIGNATURES[name][1]
        assert argtypes[-1] is C.POINTER(plan) and all(t in (C.c_int, C.c_long) for t in argtypes[:-1]), name
    assert lib.pf_groupnorm_plan(1, 4099, 320, 0, 32, _lib.PF_F16, 0, 0, None) == 1 and b"pf_groupnorm_plan: null" in lib.pf_last_error_string()
    assert lib.pf_groupnorm_bwd_plan(2, 130, 64, 0, 32, None) == 1 and b"pf_groupnorm_bwd_plan: null" in lib.pf_last_error_string()
    assert lib.pf_layernorm_plan(4096, 320, None) == 1 and b"pf_layernorm_plan: null" in lib.pf_last_error_string()


P = [0x10000 * (i + 1) for i in range(12)]                                        # fake device addresses, 16-byte aligned, never dereferenced


def _refused(status, plan, message):
    err = _lib.lib().pf_last_error_string()
    assert status == 1 and bytes(plan) == bytes(type(plan)()) and message in err, (status, err)
    return err


def test_a_refused_problem_has_no_plan_and_the_launch_refuses_it_with_the_same_message():
    lib = _lib.lib()
    F16 = _lib.PF_F16
    stats = lambda n, hw, c0, c1, g, dtype=F16, ws=1 << 30: lib.pf_groupnorm_stats(P[0], c0, P[1] if c1 else None, c1, dtype, n, hw, g, 1e-5,
                                                                                 P[2], P[3], P[4], P[5], P[6], ws, None)
    for args, message in (((1, 200, 8320, 0, 32), b"pf_groupnorm_stats: C=8320 too large"), ((0, 64, 64, 0, 32), b"pf_groupnorm_stats: bad sizes"),
                          ((1, 64, 128, 0, 65), b"pf_groupnorm_stats: bad sizes"), ((1, 64, 60, 68, 32), b"must be a multiple of 8 and of groups=32"),
                          ((1, 64, 64, 0, 24), b"must be a multiple of 8 and of groups=24"), ((1, 64, 64, 0, 32, 3), b"dtype must be")):
        g = _lib.GnPlan()
        a = args + (F16,) if len(args) == 5 else args
        err = _refused(lib.pf_groupnorm_plan(*a, 0, 0, C.byref(g)), g, message)
        assert stats(*args) == 1 and lib.pf_last_error_string() == err, args
    # moments that cannot serve: the planner falls back to the statistics pass, pf_groupnorm_from_partials itself refuses
    part = lambda n, hw, c0, r0, c1, r1, g: lib.pf_groupnorm_from_partials(P[0], c0, r0, P[1] if c1 else None, c1, r1, n, hw, g, 1e-5,
                                                                         P[2], P[3], P[4], P[5], None)
    for (n, hw, c0, r0, c1, r1, groups), message in (((2, 64, 96, 8, 0, 0, 32), b"even numbers of channels"),
                                                     ((2, 100, 128, 8, 0, 0, 32), b"an image (100 rows) must be whole runs of 8 / 8 rows"),
                                                     ((1, 64, 2560, 8, 0, 0, 2), b"C=2560 too large for 2 groups")):
        g = _lib.GnPlan()
        assert lib.pf_layernorm_plan(0, 64, None) == 1                            # (a message of another entry point: an accepted plan leaves it alone)
        assert lib.pf_groupnorm_plan(n, hw, c0, c1, groups, _lib.PF_F32, r0, r1, C.byref(g)) == 0
        assert lib.pf_groupnorm_workspace_size(n, hw, c0 + c1) == g.workspace_bytes and lib.pf_groupnorm_param_grads_workspace_size(1, 300, 8224) > 0
        assert lib.pf_last_error_string().startswith(b"pf_layernorm_plan: null")
        assert g.partials_refused == 1 and g.arm in (_lib.PF_GN_DIRECT, _lib.PF_GN_TWO_STAGE) and g.workspace_bytes > 0
        assert part(n, hw, c0, r0, c1, r1, groups) == 1 and b"pf_groupnorm_from_partials" in lib.pf_last_error_string()
        assert message in lib.pf_last_error_string()
    bwd = lambda n, hw, c0, c1, g: lib.pf_groupnorm_bwd(P[0], c0, P[1] if c1 else None, c1, F16, n, hw, g, 1e-5, P[2], P[3], P[4], 1,
                                                       P[5], None, P[6], P[7] if c1 else None, P[8], 1 << 30, None)
    par = lambda n, hw, c0, c1: lib.pf_groupnorm_param_grads(P[0], c0, P[1] if c1 else None, c1, F16, n, hw, P[2], P[3], P[4], P[5], 1,
                                                            P[6], P[7], P[8], 1 << 30, None)
    for (n, hw, c0, c1, groups), message in (((1, 300, 4128, 0, 32), b"pf_groupnorm_bwd: 4128 channels exceed the 64 KiB staging buffer"),
                                             ((0, 64, 64, 0, 32), b"pf_groupnorm_bwd: bad arguments"),
                                             ((1, 64, 64, 0, 24), b"pf_groupnorm_bwd: channels (64,0) must be multiples of 8 and divide into 24 groups"),
                                             ((65536, 1, 64, 0, 32), b"pf_groupnorm_bwd: at most 65535 images"),
                                             ((1, 300, 8224, 0, 0), b"pf_groupnorm_param_grads: 8224 channels exceed the 64 KiB staging buffer"),
                                             ((1, 64, 60, 0, 0), b"pf_groupnorm_param_grads: channels (60,0) must be multiples of 8"),
                                             ((65536, 1, 64, 0, 0), b"pf_groupnorm_param_grads: at most 65535 images")):
        g = _lib.GnBwdPlan()
        err = _refused(lib.pf_groupnorm_bwd_plan(n, hw, c0, c1, groups, C.byref(g)), g, message)
        assert (bwd(n, hw, c0, c1, groups) if groups else par(n, hw, c0, c1)) == 1 and lib.pf_last_error_string() == err
    assert bwd(1, 64, 64, 0, 0) == 1 and b"divide into 0 groups" in lib.pf_last_error_string()      # (no groups is no plan of the backward)
    for (rows, Cc), message in (((0, 64), b"pf_layernorm: bad arguments"), ((4, 2056), b"pf_layernorm: C=2056 must be a multiple of 8 and <= 2048"),
                                ((4, 60), b"pf_layernorm: C=60"), ((4, 0), b"pf_layernorm_bwd: C=0 must be a multiple of 8, at most 2048")):
        g = _lib.LnPlan()
        err = _refused(lib.pf_layernorm_plan(rows, Cc, C.byref(g)), g, message)
        if err.startswith(b"pf_layernorm:"):
            assert lib.pf_layernorm(P[0], None, 0, F16, rows, Cc, P[1], P[2], 1e-5, F16, P[3], None) == 1 and lib.pf_last_error_string() == err
        assert lib.pf_layernorm_bwd(P[0], None, 0, F16, rows, Cc, P[1], 1e-5, P[2], None, P[3], P[4], None) == 1
        assert lib.pf_last_error_string().startswith(b"pf_layernorm_bwd: " + (b"bad arguments" if rows <= 0 else b"C=%d must be" % Cc))


def test_a_workspace_one_byte_short_is_refused_before_any_launch():
    lib = _lib.lib()
    g = _lib.GnPlan()
    assert lib.pf_groupnorm_plan(1, 4099, 320, 0, 32, _lib.PF_F16, 0, 0, C.byref(g)) == 0 and g.arm == _lib.PF_GN_TWO_STAGE
    assert lib.pf_groupnorm_stats(P[0], 320, None, 0, _lib.PF_F16, 1, 4099, 32, 1e-5, P[2], P[3], P[4], P[5], P[6], g.workspace_bytes - 1, None) == 1
    assert b"pf_groupnorm_stats: workspace too small" in lib.pf_last_error_string()
    b = _lib.GnBwdPlan()
    assert lib.pf_groupnorm_bwd_plan(2, 130, 64, 0, 32, C.byref(b)) == 0 and b.ppc == 8
    assert lib.pf_groupnorm_bwd(P[0], 64, None, 0, _lib.PF_F32, 2, 130, 32, 1e-5, P[2], P[3], P[4], 1, P[5], None, P[6], None, P[8],
                                b.bwd_workspace_bytes - 1, None) == 1 and b"pf_groupnorm_bwd: workspace too small" in lib.pf_last_error_string()
    assert lib.pf_groupnorm_param_grads(P[0], 64, None, 0, _lib.PF_F32, 2, 130, P[2], P[3], P[4], P[5], 1, P[6], P[7], P[8],
                                        b.param_workspace_bytes - 1, None) == 1 and b"pf_groupnorm_param_grads: workspace too small" in lib.pf_last_error_string()


def test_ops_asks_the_plan_for_the_arm(monkeypatch):
    """ops.groupnorm_scale_shift holds no rule of its own: on tensors without storage, with the three launches replaced by recorders, it
    reaches the launch the plan names with the plan's workspace -- moments that serve, moments that cannot, no moments, a circular wrap."""
    import torch
    from panfusion_amd import ops
    lib, calls = _lib.lib(), []

    class Recorder:
        def __getattr__(self, name):
            if name in ("pf_groupnorm_stats", "pf_groupnorm_stats_wrap", "pf_groupnorm_from_partials"):
                return lambda *a: calls.append((name, a)) or 0
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "lib", lambda: Recorder())
    monkeypatch.setattr(ops, "_stream", lambda: None)
    meta = lambda *s, dtype=torch.float16: torch.empty(*s, device="meta", dtype=dtype)
    for p in G.gn_problems():
        if p["tag"] not in ("model_part", "gpb", "ragged", "two_sources", "part_refused", "model_gn") or p["c0"] % 8 or p["c1"] % 8:
            continue
        n, hw, c0, c1, groups = p["n"], p["hw"], p["c0"], p["c1"], p["groups"]
        dtype = (torch.bfloat16, torch.float16, torch.float32)[p["dtype"]]
        x0, x1 = meta(n, hw, c0, dtype=dtype), meta(n, hw, c1, dtype=dtype) if c1 else None
        if p["rows0"]:
            x0._pf_gn = (meta(n * hw // p["rows0"], 2, c0 // 2, dtype=torch.float32), p["rows0"])
        if p["rows1"]:
            x1._pf_gn = (meta(n * hw // p["rows1"], 2, c1 // 2, dtype=torch.float32), p["rows1"])
        g = _lib.GnPlan()
        assert lib.pf_groupnorm_plan(n, hw, c0, c1, groups, p["dtype"], p["rows0"], p["rows1"], C.byref(g)) == 0
        for wrap in (None, (hw, 0)) + (((8, 2),) if hw % 8 == 0 else ()):
            del calls[:]
            ops.groupnorm_scale_shift(x0, x1, n, hw, groups, 1e-5, meta(c0 + c1), meta(c0 + c1), wrap=wrap)
            (name, a), = calls
            if wrap is not None and wrap[1] > 0:
                w = _lib.GnPlan()
                assert lib.pf_groupnorm_plan(n, hw, c0, c1, groups, p["dtype"], 0, 0, C.byref(w)) == 0
                assert name == "pf_groupnorm_stats_wrap" and a[-2] == w.workspace_bytes, p
            elif g.arm == _lib.PF_GN_FROM_PARTIALS:
                assert name == "pf_groupnorm_from_partials" and (a[2], a[5]) == (p["rows0"], p["rows1"] or p["rows0"]), p
            else:
                assert name == "pf_groupnorm_stats" and a[-2] == g.workspace_bytes, p
