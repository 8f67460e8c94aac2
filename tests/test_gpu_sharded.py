"""The sharded denoising path on the real HIP kernels.

Part A (one process): the attention kernel called the way a sharded rank calls it -- a row band of the view queries with the band's
bias rows and tile-flag map (engine.run_epa_sharded), a band of the panorama's self-attention queries against all keys
(sharding.split_pano_attention) -- against a float64 reference on the same 16-bit inputs.

Part B: N ranks (tests/sharded_worker.py, one fresh process each, all on cuda:0, collectives over gloo) run one denoiser call and the
3-step loop, eager and as hipGraph segments; the parent asserts the numbers against the reference fixtures, against the
single-process HIP result, across replicas, and the collective counts.  One GPU over gloo says nothing about RCCL or scaling.
Needs an MI355X: `-m gpu`."""
import os
import signal
import socket
import subprocess
import sys
import tempfile
import time
import types

import pytest
import torch

import sharded_worker as W
from conftest import cam4, golden, rel_l2
from test_gpu_kernels import TOL as KTOL
from test_gpu_kernels import attn_ref, check, q16, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------ part A: the kernels as a sharded rank calls them
SPLITS = [(1, 3), (2, 2), (0, 2, 1, 1), (1, 1, 1, 1)]
LEVELS = [(2, 2, 2, 4), (4, 4, 4, 8), (8, 8, 8, 16)]        # (ph, pw, eh, ew) of the tiny model's three EPA levels: P = 4 / 16 / 64, E = 8 / 32 / 128


def _bands(split, P):
    """Row bands [r0, r1) of the view queries, one per view group that holds views, from the planner itself."""
    from panfusion_amd import sharding
    G = len(split)
    out = []
    for g in range(G):
        s = sharding.plan(2 * G, g, 4, split=split)
        assert s.counts == split
        v0, v1 = s.views
        if v1 > v0:
            out.append((v0 * P, v1 * P))
    return out


def test_part_a_reaches_the_band_edges():
    """At least one band starts inside a 32-row flag tile and at least one has nq % 32 != 0 (a later change of sizes must not drop them)."""
    bands = [b for ph, pw, _, _ in LEVELS for split in SPLITS for b in _bands(split, ph * pw)]
    assert any(r0 % 32 for r0, _ in bands) and any((r1 - r0) % 32 for r0, r1 in bands)
    assert any(r0 % 32 == 0 and r0 > 0 for r0, _ in bands)        # ... and the sliced (not re-derived) flag map of a later band


@pytest.fixture(scope="module")
def epa_tables():
    from panfusion_amd import ops
    c = cam4()
    out = {}
    for ph, pw, eh, ew in LEVELS:
        _, bias_p, _, flags_p = ops.epa_tables(c["FoV"], c["theta"], c["phi"], ph, pw, eh, ew, DEV)
        out[ph * pw] = (bias_p, flags_p)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("level", LEVELS, ids=lambda l: "P%d_E%d" % (l[0] * l[1], l[2] * l[3]))
def test_row_band_epa_attention_vs_float64(epa_tables, level, dtype):
    from panfusion_amd import engine, ops
    ph, pw, eh, ew = level
    P, E, m, H, D = ph * pw, eh * ew, 4, 2, 32
    C, mP = H * D, 4 * ph * pw
    ld = 2 * C
    bias_p, flags_p = epa_tables[P]
    assert bias_p.shape == (mP, E) and float(bias_p.abs().max()) > 0
    qk_p, qkf_p = q16(rnd(mP, ld, seed=50 + P), dtype)              # (q | k) of the view tokens, (q | k) of the panorama tokens
    qk_e, qkf_e = q16(rnd(E, ld, seed=51 + P), dtype)
    v, vf = q16(rnd(1, E, C, seed=52 + P), dtype)
    vt_e = torch.full((1, C, ((E + 31) // 32) * 32), float("nan"), dtype=dtype, device=DEV)     # padding must never be read as data
    vt_e[:, :, :E] = v.transpose(1, 2)
    bias64 = bias_p.cpu().double()
    ref = lambda r0, r1: attn_ref(qkf_p[r0:r1, :C][None].double(), qkf_e[:, C:][None].double(), vf.double(), H, D ** -0.5, bias64[r0:r1])
    want_full = ref(0, mP)
    for split in SPLITS:
        t = types.SimpleNamespace(bias_p=bias_p, flags_p=flags_p)   # (the helper caches re-derived maps on the table entry)
        got = []
        for r0, r1 in _bands(split, P):
            nq = r1 - r0
            flags = engine.band_flags_p(t, r0, r1)
            rows = torch.nn.functional.pad(bias_p[r0:r1], (0, (-E) % 32, 0, (-nq) % 32))
            true_map = rows.reshape(rows.shape[0] // 32, 32, rows.shape[1] // 32, 32).abs().amax((1, 3)) > 0
            assert flags.shape == true_map.shape and flags.dtype == torch.uint8 and flags.stride(-1) == 1
            if r0 % 32 == 0 and r1 % 32 and r1 < mP:         # sliced band that ends inside a tile: its last flag row also sees the next band's rows
                assert torch.equal(flags[:-1].bool(), true_map[:-1]) and bool((flags[-1:].bool() | ~true_map[-1:]).all())
            else:
                assert torch.equal(flags.bool(), true_map), (split, r0, r1)
            out = ops.attention(qk_p[r0:r1], qk_e[:, C:], vt_e, 1, H, D, nq, E, q_ld=ld, k_ld=ld, vt_ld=vt_e.shape[-1],
                                q_bs=nq * ld, k_bs=E * ld, vt_bs=vt_e.shape[1] * vt_e.shape[2],
                                bias=bias_p[r0:r1], flags=flags)
            check("band %s [%d, %d) P=%d" % (split, r0, r1, P), out, ref(r0, r1), 2.5 * KTOL[dtype])
            got.append(out)
        check("bands of %s stitched, P=%d" % (split, P), torch.cat(got, 1), want_full, 2.5 * KTOL[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("C,H", [(64, 1), (128, 2)])
@pytest.mark.parametrize("nq", [128, 512])
def test_query_split_self_attention_vs_float64(nq, C, H, G, dtype):
    """sharding.split_pano_attention's call: rank g computes the rows [g nq / G, (g + 1) nq / G) against all keys."""
    from panfusion_amd import ops
    D, ld = C // H, 2 * C
    qk, qkf = q16(rnd(nq, ld, seed=60), dtype)
    v, vf = q16(rnd(1, nq, C, seed=61), dtype)
    vt = v.transpose(1, 2).contiguous()
    rows = nq // G
    assert nq % (32 * G) == 0                                       # sharding._split_rule
    got = []
    for g in range(G):
        r0 = g * rows
        got.append(ops.attention(qk[r0:r0 + rows], qk[:, C:], vt, 1, H, D, rows, nq, q_ld=ld, k_ld=ld, vt_ld=vt.shape[-1],
                                 q_bs=rows * ld, k_bs=nq * ld, vt_bs=vt.shape[1] * vt.shape[2]).reshape(rows, C))
    want = attn_ref(qkf[:, :C][None].double(), qkf[:, C:][None].double(), vf.double(), H, D ** -0.5)
    check("query split G=%d" % G, torch.cat(got)[None], want, 2.5 * KTOL[dtype])


# ------------------------------------------------------------------------------ part B: ranks over gloo
LAUNCH_CAP_S = 300.0
_FAULTED = []           # latch: a rank ended by a signal, aborted or hung -- nothing more is started on a card that may have faulted


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tail(path, n=40):
    with open(path, errors="replace") as f:
        return "".join(f.readlines()[-n:])


def _abnormal(code):
    """Ended by a signal, aborted or segmentation fault (status 1 = a Python traceback: a clean failure)."""
    return code is not None and (code < 0 or code in (134, 139))


def _launch(world, out, dtype="fp16", precision=None, layout=None, split=None, overrides=None):
    """Start `world` ranks, poll them, return the wall time.  The first rank that ends with a non-zero status, or the time limit,
    ends the launch: every remaining rank's process group is killed and the test fails with that rank's stderr tail."""
    if _FAULTED:
        pytest.fail("not started: an earlier launch ended abnormally (%s)" % _FAULTED[0])
    env = dict(os.environ)                               # the parent's, plus only the PF_SHARD_* overrides and PYTHONPATH
    assert all(k.startswith("PF_SHARD_") for k in (overrides or {}))
    env.update({k: str(v) for k, v in (overrides or {}).items()})
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    port = _free_port()
    procs, logs = [], []
    t0 = time.monotonic()
    try:
        for r in range(world):
            cmd = [sys.executable, os.path.join(HERE, "sharded_worker.py"), "--rank", str(r), "--world", str(world), "--port", str(port),
                   "--out", out, "--dtype", dtype]
            for flag, val in (("--precision", precision), ("--layout", layout), ("--split", ",".join(map(str, split)) if split else None)):
                if val:
                    cmd += [flag, val]
            logs.append(os.path.join(out, "stderr%d.txt" % r))
            with open(logs[-1], "w") as err:
                procs.append(subprocess.Popen(cmd, env=env, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=err,
                                              start_new_session=True))
        while True:
            codes = [p.poll() for p in procs]
            if all(c == 0 for c in codes):
                return time.monotonic() - t0
            if any(c not in (None, 0) for c in codes) or time.monotonic() - t0 > LAUNCH_CAP_S:
                break
            time.sleep(0.05)
        timed_out = not any(c not in (None, 0) for c in codes)
        if not timed_out:
            # a peer of a faulted rank may be reaped first (its connection was reset): give the others a moment, then look at ALL of them
            t1 = time.monotonic()
            while any(p.poll() is None for p in procs) and time.monotonic() - t1 < 2.0:
                time.sleep(0.05)
            codes = [p.poll() for p in procs]
        faulted = [(r, c) for r, c in enumerate(codes) if _abnormal(c)]
        if timed_out:
            rank, code = next(r for r, c in enumerate(codes) if c is None), "the time limit"
        else:
            rank, code = (faulted or [(r, c) for r, c in enumerate(codes) if c not in (None, 0)])[0]
        if timed_out or faulted:
            _FAULTED.append("world %d rank %d ended with %s" % (world, rank, code))
        pytest.fail("world %d: rank %d ended with %s (all ranks: %s)\n%s" % (world, rank, code, codes, _tail(logs[rank])))
    finally:
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
        for p in procs:
            p.wait()


_SINGLE = {}


def _single(dtype, precision):
    """The single-process HIP results of the same model: one call at t = 981 and the 3-step eager loop (computed once per scheme)."""
    key = (dtype, precision)
    if key not in _SINGLE:
        from panfusion_amd.pipeline import DenoiseLoop
        try:
            model = W.build_model(getattr(torch, W.DTYPES[dtype]), precision)
            lat, pl, pe, ppe, cam1 = W.tiny_inputs(DEV)
            cams = {k: torch.cat([v, v]) for k, v in cam1.items()}
            s, ps = model(lat, pl, torch.full((2, 4), 981, dtype=torch.long, device=DEV), pe, ppe, cams)
            l3, p3 = DenoiseLoop(model, lat[:1], pl[:1], pe, ppe, cam1, steps=W.STEPS, use_graphs=False).run()
            _SINGLE[key] = dict(eps=s.cpu(), pano_eps=ps.cpu(), lat=l3.cpu(), pano=p3.cpu(), precision=model.precision)
        except RuntimeError as e:                       # a HIP error in this process: no further launch on this card either
            _FAULTED.append("the single-process run raised %s" % type(e).__name__)
            raise
    return _SINGLE[key]


# Bounds against the reference fixtures: the single call as test_denoiser_vs_reference_golden, the loop as test_three_ddim_steps_golden.
# bf16 "fast" has no loop bar in the project: the bound is 4x the measured error of the bf16 loop against the fp32 oracle loop (the margin
# for the run-to-run spread of a differently batched model), rounded up to one digit.  Measured on an MI355X: latents 2.451e-2, panorama
# 2.193e-2 -> 4 x 2.451e-2 = 9.8e-2 -> 1e-1.  It must stay below the ratio of the project's two single-step bars applied to the fp16
# loop bar (3e-2 / 1e-3 = 30x of 5e-3 = 0.15).
BF16_LOOP_CAP = 30 * 5e-3
BF16_LOOP_TOL = 1e-1
assert BF16_LOOP_TOL <= BF16_LOOP_CAP
CALL_TOL = {("fp16", "mixed"): 1e-3, ("bf16", "fast"): 3e-2}
LOOP_TOL = {("fp16", "mixed"): 5e-3, ("bf16", "fast"): BF16_LOOP_TOL}
CONSISTENCY = 2e-4                                                  # sharded vs single-process HIP

LAUNCHES = {
    # id: world, layout, split, dtype, precision, PF_SHARD_* overrides, the views per group the plan must give, query split expected
    "A": dict(world=2, counts=(4,)),
    "B": dict(world=4, layout="even", counts=(2, 2)),
    "C": dict(world=4, split=(1, 3), counts=(1, 3), overrides={"PF_SHARD_ATTN_MIN_TOKENS": 128, "PF_SHARD_ATTN_MIN_GROUP": 2}, qsplit=True),
    "D": dict(world=6, split=(0, 2, 2), counts=(0, 2, 2), dtype="bf16", precision="fast"),
    "E": dict(world=8, counts=(0, 2, 1, 1), overrides={"PF_SHARD_ATTN_MIN_TOKENS": 128, "PF_SHARD_ATTN_MIN_GROUP": 2}, qsplit=True),
}


@pytest.mark.parametrize("lid", sorted(LAUNCHES))
def test_sharded_ranks_on_the_real_kernels(lid):
    L = LAUNCHES[lid]
    world, dtype, precision, layout = L["world"], L.get("dtype", "fp16"), L.get("precision"), L.get("layout")
    G = world // 2
    with tempfile.TemporaryDirectory() as out:
        wall = _launch(world, out, dtype=dtype, precision=precision, layout=layout, split=L.get("split"), overrides=L.get("overrides"))
        res = [torch.load(os.path.join(out, "r%d.pt" % r)) for r in range(world)]
    one = _single(dtype, precision)
    scheme = (dtype, one["precision"])
    g, gd = golden("mvgen_tiny.npz"), golden("ddim3_tiny.npz")
    assert [r["counts"] for r in res] == [L["counts"]] * world and [r["cfg"] for r in res] == [r // G for r in range(world)]
    even = layout == "even" or G == 1
    assert [r["has_pano"] for r in res] == [even or r % G == 0 for r in range(world)]

    # one denoiser call: the ranks' slices assembled, against the reference fixture and against the single process
    eps = torch.stack([torch.cat([res[c * G + k]["eps"][0] for k in range(G)]) for c in range(2)])
    pano_eps = torch.cat([res[c * G]["pano_eps"] for c in range(2)])
    assert eps.shape == (2, 4, 4, 16, 16) and pano_eps.shape == (2, 1, 4, 16, 32)
    assert all((r["pano_eps"] is not None) == r["has_pano"] for r in res)
    fig = dict(call_views=rel_l2(eps, torch.from_numpy(g["sample"])), call_pano=rel_l2(pano_eps, torch.from_numpy(g["pano_sample"])),
               call_views_vs_single=rel_l2(eps, one["eps"]), call_pano_vs_single=rel_l2(pano_eps, one["pano_eps"]))
    # the loop: every rank against the fixture and the single process (replicas are compared bit for bit below)
    want_l, want_p = torch.from_numpy(gd["latents"]), torch.from_numpy(gd["pano_latent"])
    runs = [r[kind] for r in res for kind in ("eager", "graphed")]
    fig.update(loop_views=max(rel_l2(x[0], want_l) for x in runs), loop_pano=max(rel_l2(x[1], want_p) for x in runs),
               loop_views_vs_single=max(rel_l2(x[0], one["lat"]) for x in runs),
               loop_pano_vs_single=max(rel_l2(x[1], one["pano"]) for x in runs),
               single_loop_views=rel_l2(one["lat"], want_l), single_loop_pano=rel_l2(one["pano"], want_p))
    print("launch %s (world %d, %s %s, views %s): wall %.1f s  " % (lid, world, dtype, scheme[1], "/".join(map(str, L["counts"])), wall)
          + "  ".join("%s %.3e" % kv for kv in fig.items()))
    assert fig["call_views"] <= CALL_TOL[scheme] and fig["call_pano"] <= CALL_TOL[scheme], fig
    assert fig["loop_views"] <= LOOP_TOL[scheme] and fig["loop_pano"] <= LOOP_TOL[scheme], fig

    # replicas: every rank holds the same bits, eager and graphed; a rank's graphed run equals its eager run
    for kind in ("eager", "graphed"):
        assert all(torch.equal(res[0][kind][0], r[kind][0]) and torch.equal(res[0][kind][1], r[kind][1]) for r in res[1:]), kind
    for r in res:
        assert torch.equal(r["eager"][0], r["graphed"][0]) and torch.equal(r["eager"][1], r["graphed"][1])
    assert all(r["use_graphs"] for r in res), "a capture failed somewhere: the ranks fell back to eager launches"
    assert all(r["async"] for r in res)

    # sharded vs single-process HIP: a consistency check below the reference bounds
    for k in ("call_views_vs_single", "call_pano_vs_single", "loop_views_vs_single", "loop_pano_vs_single"):
        assert fig[k] <= CONSISTENCY, (k, fig)

    # collectives of the graphed loop, per step
    for r in res:
        comm = r["comm"]
        if world > 2:
            assert comm["all_gather view tokens (EPA, group of %d)" % G]["calls_per_step"] == 7
            assert ("broadcast panorama tokens (EPA, group of %d)" % G in comm) == (layout != "even")
            if layout != "even":
                assert comm["broadcast panorama tokens (EPA, group of %d)" % G]["calls_per_step"] == 7
        else:
            assert not any("EPA" in k for k in comm)
        assert comm["all_gather eps views (world)"]["calls_per_step"] == 1 and comm["all_gather eps panorama (world)"]["calls_per_step"] == 1
        assert comm["all_gather eps panorama (world)"]["bytes_per_rank_per_call"] == one["pano"].numel() * 4
        qkeys = [k for k in comm if "query split" in k]
        if L.get("qsplit"):
            n_split = res[0]["comm"]["all_gather panorama attention rows (query split, group of %d)" % G]["calls_per_step"]
            assert n_split >= 5 and n_split == int(n_split)
            assert comm["all_gather panorama attention rows (query split, group of %d)" % G]["calls_per_step"] == n_split
            assert comm["broadcast panorama self-attention tokens (query split, group of %d)" % G]["calls_per_step"] == n_split
        else:
            assert not qkeys, qkeys
