"""pf_attention plans one problem in one place: pf_attention_plan, of which pf_attention_workspace_size is a projection and which the
launch itself resolves.  The plans of a fixed grid of problems (tests/attention_plan_grid.py) under every dispatch-relevant setting of
the PF_ATTENTION_* knobs must equal tests/golden/attention_plans.npz row for row; the fixture's parent_workspace_size came from the
library as it was before the planner existed (tools/make_golden_attention_plans.py).  Host arithmetic on fake pointers: no GPU.

One deliberate difference from that older library: it sized scratch from the shape alone, also for problems its launch then ran on the
no-LDS kernel, which never splits (PF_ATTENTION_IMPL=direct, a V^T layout that is not 16-byte aligned) -- scratch the launch ignored.
The plan reports 0 bytes there; on every other row the query equals the older library's."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import attention_model as M
import attention_plan_grid as G
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


def test_plans_equal_the_fixture_row_for_row():
    fx = np.load(os.path.join(GOLDEN, "attention_plans.npz"))
    probs = G.problems()
    assert tuple(fx["columns"]) == G.COLUMNS and tuple(fx["envs"]) == tuple(repr(e) for e in G.ENVS)
    assert tuple(fx["problems"]) == tuple(repr(p) for p in probs)
    tab, want = current_table(), fx["table"]
    assert tab.shape == want.shape
    bad = np.argwhere((tab != want).any(axis=2))
    assert len(bad) == 0, "%d rows differ; first: setting %s, problem %s: got %s, fixture %s" % (
        len(bad), G.ENVS[bad[0][0]], probs[bad[0][1]], dict(zip(G.COLUMNS, tab[tuple(bad[0])])), dict(zip(G.COLUMNS, want[tuple(bad[0])])))
    # the query of the library before the planner: equal wherever a launch can split at all (see the module docstring)
    parent, no_lds = fx["parent_workspace_size"], col(tab, "kernel") == 0
    assert (col(tab, "workspace_size")[~no_lds] == parent[~no_lds]).all()
    assert (col(tab, "workspace_size")[no_lds] == 0).all() and (parent[no_lds] > 0).any()


def test_query_is_a_projection_and_plans_are_consistent():
    tab = current_table()
    ws, S, tiles = col(tab, "workspace_bytes"), col(tab, "splits"), col(tab, "split_tiles")
    assert (col(tab, "workspace_size") == ws).all()
    assert ((ws > 0) == (S > 1)).all() and (S > 1).any()
    P = G.problems()
    nkt = np.array([(p["nk"] + 63) // 64 for p in P])[None, :]
    on = S > 1
    assert (tiles[on] % 2 == 0).all() and (tiles[~on] == 0).all()
    nkt_b = np.broadcast_to(nkt, S.shape)
    assert ((S * tiles)[on] >= nkt_b[on]).all() and (nkt_b[on] > ((S - 1) * tiles)[on]).all()
    # scratch: S normalised 16-bit partial outputs + their fp32 log-sum-exps
    rows_ = np.broadcast_to(np.array([p["B"] * p["nq"] * p["H"] for p in P])[None, :], S.shape)
    D = np.broadcast_to(np.array([p["D"] for p in P])[None, :], S.shape)
    assert (ws[on] == (S * rows_ * (2 * D + 4))[on]).all()
    # instantiation fields only for k_attention_lds; block shape by kernel; the grid follows from both
    k = col(tab, "kernel")
    lds, pp = k == 1, (k == 2) | (k == 3)
    for f in ("pipelined", "occupancy", "msum"):
        assert (col(tab, f)[~lds] == 0).all()
    assert (col(tab, "occupancy")[lds] >= 2).all() and (S[~lds] == 1).all()
    assert (col(tab, "block_queries") == np.where(pp, 256, 128)).all() and (col(tab, "threads") == np.where(pp, 512, 256)).all()
    B, H, nq = (np.broadcast_to(np.array([p[f] for p in P])[None, :], S.shape) for f in ("B", "H", "nq"))
    qb = -(-nq // col(tab, "block_queries"))
    assert (col(tab, "grid_x") == np.where(k == 0, qb, qb * H * B)).all()
    assert (col(tab, "grid_y") == np.where(k == 0, H, S)).all() and (col(tab, "grid_z") == np.where(k == 0, B, 1)).all()


def test_every_launch_line_has_a_member():
    tab, P = current_table(), G.problems()
    seen = {G.plan_class(p, g) for e in range(len(G.ENVS)) for p, g in zip(P, plans(tab, e))}
    assert sorted(c for c in G.CLASSES if c not in seen) == [] and sorted(c for c in seen if c not in G.CLASSES) == []


ARMS = {"d64": (1, 0, 3, 0), "d64msum": (1, 0, 3, 1), "d32": (1, 0, 4, 0), "d32bias": (1, 0, 4, 0), "d32split": (1, 0, 4, 0), "d64bias": (1, 1, 2, 0)}


def test_every_forward_case_plans_to_the_arm_it_claims():
    """attention_model.FWD_CASES states arm, msum and split count of every case -- the error bounds of
    tests/test_gpu_attention_bounds.py follow the rounding model of that arm."""
    tab = current_table()
    env = {repr(e): i for i, e in enumerate(G.ENVS)}
    default, nosplit = plans(tab, env["{}"]), plans(tab, env[repr({"PF_ATTENTION_SPLIT": "0"})])
    for i, c in enumerate(M.FWD_CASES):
        assert G.problems()[i]["tag"] == "fwd:" + c.name
        g = plans(tab, env[repr({"PF_ATTENTION_PP": str(c.pp)})])[i] if c.pp else default[i]
        got = (g["kernel"], g["pipelined"], g["occupancy"], g["msum"], g["splits"])
        if c.arm == "direct":
            assert (g["kernel"], g["splits"]) == (0, 1), (c.name, g)
        elif c.arm == "pp":
            assert (g["kernel"], g["splits"]) == (1 + c.pp, 1), (c.name, g)
        else:
            assert got == ARMS[c.arm] + (c.S,), (c.name, g)
            assert nosplit[i]["splits"] == 1 and (nosplit[i]["kernel"], nosplit[i]["occupancy"]) == (g["kernel"], g["occupancy"])
        assert bool(g["msum"]) == c.msum or c.arm == "pp", (c.name, g)          # (pp: the denominator on the matrix pipe, as MSUM)
        assert (c.S > 1) == (c.arm == "d32split")


def test_bad_descriptors_have_no_plan():
    lib = _lib.lib()
    g = _lib.AttnPlan()
    ok = G.descriptor(**G.problems()[0])
    assert lib.pf_attention_plan(C.byref(ok), C.byref(g)) == 0
    assert lib.pf_attention_plan(None, C.byref(g)) == 1 and lib.pf_attention_plan(C.byref(ok), None) == 1
    for f, v in (("B", 0), ("H", -1), ("nq", 0), ("nk", 0), ("D", 48), ("D", 128)):
        d = G.descriptor(**G.problems()[0])
        setattr(d, f, v)
        assert lib.pf_attention_plan(C.byref(d), C.byref(g)) == 1, (f, v)
        assert b"pf_attention_plan" in lib.pf_last_error_string()
        assert lib.pf_attention_workspace_size(C.byref(d)) == 0
    assert lib.pf_attention_workspace_size(None) == 0


# ------------------------------------------------------------------------------------------------ the shared validator
def _desc(wide, **kw):
    """A structurally valid problem of pf_attention (D = 64) or pf_attention_wide (D = 128) on fake addresses; kw overrides fields."""
    a = _lib.AttnDesc()
    a.q, a.k, a.vt, a.out = 0x10000, 0x20000, 0x30000, 0x40000
    a.dtype, a.B, a.H, a.D, a.nq, a.nk = _lib.PF_F16, 2, 2, (128 if wide else 64), 100, 77
    a.q_ld = a.k_ld = a.o_ld = a.H * a.D
    a.vt_ld = 96
    a.q_bs, a.k_bs, a.vt_bs, a.o_bs = 100 * a.q_ld, 77 * a.k_ld, a.q_ld * 96, 100 * a.o_ld
    a.scale = 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


SHARED_RULES = [
    (dict(q=0), b"null pointer"), (dict(k=0), b"null pointer"), (dict(vt=0), b"null pointer"), (dict(out=0), b"null pointer"),
    (dict(B=0), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(nq=0), b"bad sizes"), (dict(nk=-1), b"bad sizes"),
    (dict(q_ld=1028), b"leading dimensions"), (dict(k_ld=1028), b"leading dimensions"), (dict(o_ld=1026), b"leading dimensions"),
    (dict(vt_ld=98), b"leading dimensions"),
    (dict(q_ld=64), b"cover H * D"), (dict(k_ld=120), b"cover H * D"), (dict(o_ld=124), b"cover H * D"),
    (dict(vt_ld=64), b"vt_ld=64 must cover nk=77"),
    (dict(q_bs=100 * 1024 + 4), b"batch strides"), (dict(k_bs=4), b"batch strides"), (dict(vt_bs=96 * 1024 + 2), b"batch strides"),
    (dict(o_bs=100 * 1024 + 2), b"batch strides"),
    (dict(q=0x10008), b"16-byte aligned"), (dict(k=0x20004), b"16-byte aligned"), (dict(vt=0x30002), b"16-byte aligned"), (dict(out=0x40008), b"16-byte aligned"),
    (dict(bias=0x50000), b"bias and flags come together"), (dict(flags=0x60000), b"bias and flags come together"),
]


@pytest.mark.parametrize("wide", [False, True], ids=["pf_attention", "pf_attention_wide"])
def test_both_entry_points_share_the_layout_rules(wide):
    """Each rule: PF_ERR_ARG with the entry point's name and the rule's message, before any launch (no GPU here: a launch would fail
    differently)."""
    lib = _lib.lib()
    fn, who = (lib.pf_attention_wide, b"pf_attention_wide: ") if wide else (lib.pf_attention, b"pf_attention: ")
    for kw, needle in SHARED_RULES:
        assert fn(C.byref(_desc(wide, **kw)), None) == 1, kw
        msg = lib.pf_last_error_string()
        assert msg.startswith(who) and needle in msg, (kw, msg)
    assert fn(None, None) == 1 and lib.pf_last_error_string() == who + b"null descriptor"


def test_attention_refuses_a_grid_that_cannot_be_launched():
    lib = _lib.lib()
    # k_attention_lds: 1-D grid of 2^24 workgroups x 256 threads = 2^32 threads (the limit is 2^32 - 1)
    big = dict(B=1 << 12, H=1, D=64, nq=(1 << 12) * 128, q_ld=64, k_ld=64, o_ld=64, q_bs=0, k_bs=0, vt_bs=0, o_bs=0)
    assert lib.pf_attention(C.byref(_desc(False, **big)), None) == 1
    msg = lib.pf_last_error_string()
    assert msg.startswith(b"pf_attention: ") and b"exceed the grid" in msg, msg
    # k_attention (a V^T layout that is 4 mod 8): heads in grid y
    many = dict(H=65536, D=32, q_ld=65536 * 32, k_ld=65536 * 32, o_ld=65536 * 32, vt_ld=100, vt_bs=0, q_bs=0, k_bs=0, o_bs=0)
    assert lib.pf_attention(C.byref(_desc(False, **many)), None) == 1 and b"exceed the grid" in lib.pf_last_error_string()
