"""pf_attention_bwd plans one problem in one place: pf_attention_bwd_plan, of which pf_attention_bwd_workspace_size is a projection and
which the launch itself resolves.  The plans of a fixed grid of problems (tests/attn_bwd_plan_grid.py) under every setting of the two
PF_ATTN_BWD_* knobs must equal tests/golden/attn_bwd_plans.npz row for row; the fixture's parent_workspace_size came from the library as
it was before the planner existed (tools/make_golden_attn_bwd_plans.py) and equals the query on EVERY row: the scratch size is a
function of qsplit, so that column pins the split of every problem against the older library.  Host arithmetic on fake pointers: no GPU."""
import ctypes as C
import functools
import os

import numpy as np

import attention_model as M
import attn_bwd_plan_grid as G
from conftest import GOLDEN
from panfusion_amd import _lib


@functools.lru_cache(maxsize=1)
def current_table():
    tab = G.table()
    tab.setflags(write=False)
    return tab


def col(tab, name):
    return tab[:, :, G.COLUMNS.index(name)]


def plans(tab, e):
    """problem index -> dict of plan fields under setting e"""
    return [dict(zip(G.PLAN_FIELDS, r[1:])) for r in tab[e]]


def per_problem(f, shape):
    return np.broadcast_to(np.array([p[f] for p in G.problems()])[None, :], shape)


def test_plans_equal_the_fixture_row_for_row():
    fx = np.load(os.path.join(GOLDEN, "attn_bwd_plans.npz"))
    probs = G.problems()
    assert tuple(fx["columns"]) == G.COLUMNS and tuple(fx["envs"]) == tuple(repr(e) for e in G.ENVS)
    assert tuple(fx["problems"]) == tuple(repr(p) for p in probs)
    tab, want = current_table(), fx["table"]
    assert tab.shape == want.shape
    bad = np.argwhere((tab != want).any(axis=2))
    assert len(bad) == 0, "%d rows differ; first: setting %s, problem %s: got %s, fixture %s" % (
        len(bad), G.ENVS[bad[0][0]], probs[bad[0][1]], dict(zip(G.COLUMNS, tab[tuple(bad[0])])), dict(zip(G.COLUMNS, want[tuple(bad[0])])))
    # the query of the library before the planner, on every row
    parent = fx["parent_workspace_size"]
    assert parent.shape == col(tab, "workspace_size").shape and (col(tab, "workspace_size") == parent).all() and (parent > 0).any()


def test_query_is_a_projection_and_plans_are_consistent():
    tab = current_table()
    ws, qs, k = col(tab, "workspace_bytes"), col(tab, "qsplit"), col(tab, "kernel")
    assert (col(tab, "workspace_size") == ws).all()
    split = qs > 1
    assert ((ws > 0) == split).all() and ((col(tab, "reduce_grid_x") > 0) == split).all() and split.any()
    assert (k[split] == 2).all() and (qs >= 1).all()
    B, H, D, nq, nk = (per_problem(f, qs.shape) for f in ("B", "H", "D", "nq", "nk"))
    assert (ws == np.where(split, 2 * qs * B * nk * H * D * 4, 0)).all()
    # the split rule: towards 512 blocks, at least 8 query tiles per block, never with 384 blocks or more
    base = -(-nk // 128) * H * B
    assert (base[split] < 384).all() and (qs <= np.maximum(1, (nq // 32) // 8)).all() and (qs <= np.maximum(1, -(-512 // base))).all()
    # the grids follow from the shapes
    assert (col(tab, "threads") == 256).all()
    for f, want in (("dq_grid_x", -(-nq // 128)), ("dq_grid_y", H), ("dq_grid_z", B), ("dkv_grid_x", -(-nk // 128) * qs), ("dkv_grid_y", H),
                    ("dkv_grid_z", B), ("reduce_grid_x", np.where(split, -(-(B * nk * H * D // 4) // 256), 0)),
                    ("reduce_grid_y", split.astype(np.int64)), ("reduce_grid_z", split.astype(np.int64))):
        assert (col(tab, f) == want).all(), f
    # the arms: ragged token counts take the guarded kernels under every setting, nothing is LDS-staged or split under IMPL=direct,
    # nothing is split under QSPLIT=0 and the kernels are those of the defaults
    env = {repr(e): i for i, e in enumerate(G.ENVS)}
    ragged = (nq % 32 != 0) | (nk % 32 != 0)
    assert ((k == 1) == ragged).all()
    direct, noqs = env[repr({"PF_ATTN_BWD_IMPL": "direct"})], env[repr({"PF_ATTN_BWD_QSPLIT": "0"})]
    assert (k[direct] != 2).all() and (qs[noqs] == 1).all() and (k[noqs] == k[env["{}"]]).all()


def test_every_launch_line_has_a_member():
    tab, P = current_table(), G.problems()
    seen = {G.plan_class(p, g) for e in range(len(G.ENVS)) for p, g in zip(P, plans(tab, e))}
    assert sorted(c for c in G.CLASSES if c not in seen) == [] and sorted(c for c in seen if c not in G.CLASSES) == []


ARMS = {"whole": 0, "ragged": 1, "lds": 2, "qsplit": 2}


def test_every_backward_case_plans_to_the_arm_it_claims():
    """attention_model.BWD_CASES states the arm and the query split of every case -- the error bounds of
    tests/test_gpu_attention_bounds.py belong to those arms."""
    default = plans(current_table(), 0)
    assert G.ENVS[0] == {}
    for i, c in enumerate(M.BWD_CASES):
        assert G.problems()[i]["tag"] == "bwd:" + c.name
        g = default[i]
        assert (g["kernel"], g["qsplit"]) == (ARMS[c.arm], c.qs), (c.name, g)
        assert (c.qs > 1) == (c.arm == "qsplit")


def test_bad_descriptors_have_no_plan():
    lib = _lib.lib()
    g = _lib.AttnBwdPlan()
    ok = G.descriptor(**G.problems()[0])
    assert lib.pf_attention_bwd_plan(C.byref(ok), C.byref(g)) == 0
    assert lib.pf_attention_bwd_plan(None, C.byref(g)) == 1 and lib.pf_attention_bwd_plan(C.byref(ok), None) == 1
    for f, v in (("B", 0), ("H", -1), ("nq", 0), ("nk", 0), ("D", 48), ("D", 128)):
        d = G.descriptor(**G.problems()[0])
        setattr(d, f, v)
        assert lib.pf_attention_bwd_plan(C.byref(d), C.byref(g)) == 1, (f, v)
        assert b"pf_attention_bwd_plan" in lib.pf_last_error_string()
        assert lib.pf_attention_bwd_workspace_size(C.byref(d)) == 0
    assert lib.pf_attention_bwd_workspace_size(None) == 0


# ------------------------------------------------------------------------------------------------ the validator
def _desc(**kw):
    """A structurally valid problem (B 2, H 2, D 32, 100 queries, 76 keys, a bias) on fake addresses; kw overrides fields."""
    d = G.descriptor(**G.prob("rule", 2, 2, 32, 100, 76, bias=True))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


POINTERS = ("q", "k", "v", "dout", "qt", "kt", "dot", "dq", "dk", "dv", "lse", "delta")
RULES = (
    [(dict([(f, 0)]), b"null pointer") for f in POINTERS] +
    [(dict(D=48), b"head dim 48 unsupported"), (dict(D=128), b"head dim 128 unsupported")] +
    [(dict(B=0), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(nq=0), b"bad sizes"), (dict(nk=-4), b"bad sizes")] +
    [(dict([(f, 68)]), b"row-major leading dimensions must be multiples of 8") for f in ("q_ld", "k_ld", "v_ld", "do_ld")] +
    [(dict(qt_ld=102), b"transposed leading dimensions"), (dict(kt_ld=78), b"transposed leading dimensions"), (dict(dot_ld=102), b"transposed leading dimensions"),
     (dict(qt_ld=96), b"cover the token count"), (dict(kt_ld=72), b"cover the token count"), (dict(dot_ld=96), b"cover the token count")] +
    [(dict([(f, 66)]), b"output leading dimensions must be multiples of 4") for f in ("dq_ld", "dk_ld", "dv_ld")] +
    [(dict([(f, 6404)]), b"batch strides misaligned") for f in ("q_bs", "k_bs", "v_bs", "do_bs")] +
    [(dict([(f, 6402)]), b"batch strides misaligned") for f in ("qt_bs", "kt_bs", "dot_bs", "dq_bs", "dk_bs", "dv_bs")] +
    [(dict([(f, 0x100000 * (i + 1) + 8)]), b"pointers must be 16-byte aligned") for i, f in enumerate(POINTERS)] +
    [(dict(bias=0), b"bias and flags come together"), (dict(flags=0), b"bias and flags come together")] +
    [(dict(nk=74, kt_ld=80), b"bias needs nk % 4 == 0"), (dict(bias_ld=78), b"bias needs nk % 4 == 0"), (dict(bias_ld=72), b"bias needs nk % 4 == 0"),
     (dict(bias=0x5000008), b"bias needs nk % 4 == 0"), (dict(flags_ld=2), b"flags_ld too small")] +
    # new with the planner: rows that do not cover the H * D = 64 columns; grids HIP cannot launch
    [(dict([(f, 56)]), b"must cover H * D = 64 columns") for f in ("q_ld", "k_ld", "v_ld", "do_ld")] +
    [(dict([(f, 60)]), b"must cover H * D = 64 columns") for f in ("dq_ld", "dk_ld", "dv_ld")] +
    [(dict(B=65536), b"exceed the grid limits"),
     (dict(H=65536, q_ld=1 << 21, k_ld=1 << 21, v_ld=1 << 21, do_ld=1 << 21, dq_ld=1 << 21, dk_ld=1 << 21, dv_ld=1 << 21), b"exceed the grid limits")])


def test_each_rule_refuses_before_any_launch():
    """Each rule: PF_ERR_ARG with the entry point's name and the rule's message, before any launch (no GPU here: a launch would fail
    differently)."""
    lib = _lib.lib()
    for kw, needle in RULES:
        assert lib.pf_attention_bwd(C.byref(_desc(**kw)), None) == 1, kw
        msg = lib.pf_last_error_string()
        assert msg.startswith(b"pf_attention_bwd: ") and needle in msg, (kw, msg)
    assert lib.pf_attention_bwd(None, None) == 1 and lib.pf_last_error_string() == b"pf_attention_bwd: null descriptor"
    # the scratch of a split launch: too small or misaligned is an error, not a silent fallback
    d = G.descriptor(**G.prob("rule", 1, 2, 64, 512, 128))
    need = lib.pf_attention_bwd_workspace_size(C.byref(d))
    assert need > 0
    for ws, nbytes in ((0x7000000, need - 4), (0x7000008, need)):
        d.workspace, d.workspace_bytes = ws, nbytes
        assert lib.pf_attention_bwd(C.byref(d), None) == 1 and b"workspace too small or misaligned" in lib.pf_last_error_string()
