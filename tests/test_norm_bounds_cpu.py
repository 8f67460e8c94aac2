"""The per-element checks of tests/norm_model.py for the GroupNorm / LayerNorm kernels, exercised without a GPU: the case
tables reach the arms they name, the summation-order emulation stays inside the derived bounds and the caps on every case of
tests/test_gpu_norm_bounds.py, the recorded maxima are the emulation's, seeded local defects are flagged (and the rel-L2
tolerance of the suite accepts several of them), and the hard bound is not hollow."""
import functools

import pytest
import torch

import norm_model as M
from conftest import rel_l2

SEEN = dict(direct=0.0, two_stage=0.0, partials_scale=0.0, partials_shift=0.0, layernorm=0.0, runs=0)
GN_IDS = [c.name for c in M.GN_CASES]
LN_IDS = [c.name for c in M.LN_CASES]
N_RUNS = 3 * len(M.GN_CASES) + len(M.PART_CASES) + len(M.LN_TYPES) * len(M.LN_CASES)


# ------------------------------------------------------------------------------------------------ the tables reach their arms
def test_case_tables_reach_the_arms():
    by = {c.name: c for c in M.GN_CASES}
    for c in M.GN_CASES:
        assert c.arm == ("direct" if c.kind == "direct" else "two_stage"), c.name
        assert c.n * c.hw * (c.c0 + c.c1) <= 6.5e6, c.name
        if c.kind == "two_stage":                                       # reached through hw * cpg, not through the element cap
            assert c.hw * ((c.c0 + c.c1) // c.groups) > 32768, c.name
        if c.kind == "two_stage_cap":
            assert c.hw * ((c.c0 + c.c1) // c.groups) <= 32768, c.name
    c = by["two_stage-1x4099x320-g32"]
    assert (M.gn_ppc(1, 4099), M.gn_pix_par(320), 4099 % 17) == (17, 6, 2)          # ragged last chunk, 240 of 256 threads hold a slot
    assert (M.gn_ppc(1, 16411), M.gn_pix_par(64)) == (65, 32)                       # slots with 3 and with 2 pixels
    assert M.gn_pix_par(2560) == 1 and 2560 // 8 > 256                              # two `ob` rounds
    assert (M.gn_ppc(40, 8190), M.gn_pix_par(16)) == (64, 128)                      # pix_par > ppc
    assert M.gn_ppc(1, 64 * 132) == 33 and M.gn_ppc(1, 65 * 132) == 34 and 132 % 34 != 0      # chunks straddle image rows
    assert {c.wrap for c in M.GN_CASES if c.wrap} == {(16, 2), (8, 4), (132, 2)}
    usable = [c for c in M.PART_CASES if c.usable]
    assert {c.gpb for c in usable} == {8, 4, 2, 1}
    assert any(c.slices == 1 and c.npairs > 256 for c in usable) and any(c.slices == 1 and 128 < c.npairs <= 256 for c in usable)
    assert any(c.slices > 1 and 256 % c.npairs for c in usable) and any(c.c1 and c.rows0 != c.rows1 for c in usable)
    assert [c.name for c in M.PART_CASES if not c.usable] == ["refused-odd-cpg", "refused-rows"]
    assert {(c.rpw, c.C) for c in M.LN_CASES} >= {(4, 8), (4, 64), (4, 320), (4, 512), (1, 8), (1, 520), (1, 1280), (1, 2048)}
    assert all(c.rpw == (4 if c.C <= 512 and c.rows >= 4096 else 1) for c in M.LN_CASES)
    assert len(M.APPLY_COMBOS) == 13


def test_the_restated_dispatch_is_the_librarys():
    """norm_model restates the host dispatch by hand, and the chain lengths L of every bound come from that restatement.  Held against the
    library's own plans (host arithmetic, no GPU) -- arm, ppc, pix_par, gpb, slices, usable, rows per wave -- on every case of the three
    tables and on the whole grid of tests/norm_plan_grid.py: a dispatch constant that moves in the library moves this."""
    import ctypes as C

    import norm_plan_grid as G
    from panfusion_amd import _lib
    lib = _lib.lib()
    ARM = {_lib.PF_GN_DIRECT: "direct", _lib.PF_GN_TWO_STAGE: "two_stage"}

    def stats(n, hw, c0, c1, groups, dtype=_lib.PF_F16, rows0=0, rows1=0):
        g = _lib.GnPlan()
        return lib.pf_groupnorm_plan(n, hw, c0, c1, groups, dtype, rows0, rows1, C.byref(g)), g

    def check_stats(g, n, hw, Cc, groups, what):
        assert ARM[g.arm] == M.gn_arm(n, hw, Cc, groups), what
        if g.arm == _lib.PF_GN_TWO_STAGE:
            assert (g.ppc, g.pix_par) == (M.gn_ppc(n, hw), M.gn_pix_par(Cc)), what

    def check_partials(g, n, hw, c0, rows0, c1, rows1, groups, what):
        usable = M.partials_usable(hw, rows0, rows1, c0, c0 + c1, groups)
        assert (g.arm == _lib.PF_GN_FROM_PARTIALS) == usable and g.partials_refused == (not usable), what
        if usable:
            c = M.part_case("", n, hw, c0, rows0, c1, rows1 if c1 else 0, groups)
            assert (g.gpb, g.pairs_per_block, g.slices) == (c.gpb, c.npairs, c.slices), what
        else:
            check_stats(g, n, hw, c0 + c1, groups, what)

    for c in M.GN_CASES:
        status, g = stats(c.n, c.hw, c.c0, c.c1, c.groups)
        assert status == 0 and ARM[g.arm] == c.arm, c.name
        check_stats(g, c.n, c.hw, c.c0 + c.c1, c.groups, c.name)
        assert c.L == (M.cdiv(c.hw * ((c.c0 + c.c1) // c.groups), 256) + 6 if c.arm == "direct" else M.cdiv(g.ppc, g.pix_par) + g.pix_par * ((c.c0 + c.c1) // c.groups)), c.name
    for c in M.PART_CASES:
        status, g = stats(c.n, c.hw, c.c0, c.c1, c.groups, _lib.PF_F32, c.rows0, c.rows1 if c.c1 else 0)
        assert status == 0 and (g.arm == _lib.PF_GN_FROM_PARTIALS) == c.usable and (g.gpb, g.slices) == (c.gpb, c.slices), c.name
        check_partials(g, c.n, c.hw, c.c0, c.rows0, c.c1, c.rows1, c.groups, c.name)
    for c in M.LN_CASES:
        g = _lib.LnPlan()
        assert lib.pf_layernorm_plan(c.rows, c.C, C.byref(g)) == 0 and g.rows_per_wave == c.rpw == M.ln_rows_per_wave(c.rows, c.C), c.name
    seen = dict(stats=0, partials=0, ln=0)
    for p in G.gn_problems():
        status, g = stats(p["n"], p["hw"], p["c0"], p["c1"], p["groups"], p["dtype"], p["rows0"], p["rows1"])
        if status != 0:                                   # (the model has no notion of a refused problem)
            continue
        if p["rows0"] and (p["rows1"] or not p["c1"]):
            check_partials(g, p["n"], p["hw"], p["c0"], p["rows0"], p["c1"], p["rows1"] or p["rows0"], p["groups"], p)
            seen["partials"] += 1
        else:
            check_stats(g, p["n"], p["hw"], p["c0"] + p["c1"], p["groups"], p)
            seen["stats"] += 1
    for p in G.ln_problems():
        g = _lib.LnPlan()
        if lib.pf_layernorm_plan(p["rows"], p["C"], C.byref(g)) == 0:
            assert g.rows_per_wave == M.ln_rows_per_wave(p["rows"], p["C"]), p
            seen["ln"] += 1
    assert seen["stats"] >= 60 and seen["partials"] >= 25 and seen["ln"] >= 35, seen


# ------------------------------------------------------------------------------------------------ the emulation inside the bounds
def gn_check(name, sc, sh, ref, c, x):
    dS, dH = M.gn_stat_bounds(ref, c.L, x.gamma, x.beta)
    a = M.assert_within(name + " scale", sc, ref.scale, dS)
    b = M.assert_within(name + " shift", sh, ref.shift, dH)
    return max(a, b), M.assert_cap(name, sc, ref, c.arm)


@pytest.mark.parametrize("dtype", M.ALL3, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("i", range(len(M.GN_CASES)), ids=GN_IDS)
def test_groupnorm_emulation_within_bounds(i, dtype):
    c, x, ref = M.gn_ref(i, dtype)
    SEEN["runs"] += 1
    for fma in (False, True):
        sc, sh = M.emulate_groupnorm(x.x.float(), c.groups, x.gamma, x.beta, c.wrap, fma)
        ratio, ex = gn_check("%s %s fma%d" % (c.name, M.DT_ID[dtype], fma), sc, sh, ref, c, x)
        SEEN[c.arm] = max(SEEN[c.arm], ex)
    cg = M.const_group_of(c.groups)
    assert float(ref.var[0, cg]) == 0.0 and float(ref.kappa[0, cg]) > 1e6            # the constant group: the clamp decides


@pytest.mark.parametrize("i", range(len(M.PART_CASES)), ids=[c.name for c in M.PART_CASES])
def test_partials_emulation_within_bounds(i):
    c = M.PART_CASES[i]
    x = M.part_inputs(c, seed=i)
    SEEN["runs"] += 1
    if not c.usable:                                      # the statistics pass over the tensor serves: its bounds
        ref = M.gn_reference(x.x, c.groups, x.gamma, x.beta)
        arm, L = M.gn_chain(c.n, c.hw, c.c0 + c.c1, c.groups)
        sc, sh = M.emulate_groupnorm(x.x, c.groups, x.gamma, x.beta)
        dS, dH = M.gn_stat_bounds(ref, L, x.gamma, x.beta)
        M.assert_within(c.name + " scale", sc, ref.scale, dS)
        M.assert_within(c.name + " shift", sh, ref.shift, dH)
        return
    parts = [M.make_partials(x.x0, c.rows0)] + ([M.make_partials(x.x1, c.rows1)] if c.c1 else [])
    cs = [c.c0] + ([c.c1] if c.c1 else [])
    ref = M.partials_reference(parts, cs, c.n, c.hw, c.groups, x.gamma, x.beta)
    exact = M.gn_reference(x.x, c.groups, x.gamma, x.beta)
    assert float(((ref.scale - exact.scale).abs() / exact.scale.abs() / exact.per_c(exact.kappa)).max()) < 4 * M.U32      # (fp32 partials: u kappa)
    dS, dH = M.partials_bounds(ref, max(c.hw // c.rows0, c.hw // c.rows1), x.beta)
    for fma in (False, True):
        sc, sh = M.emulate_partials(parts, cs, c.n, c.hw, c.groups, x.gamma, x.beta, fma)
        M.assert_within(c.name + " scale", sc, ref.scale, dS)
        SEEN["partials_shift"] = max(SEEN["partials_shift"], M.assert_within(c.name + " shift", sh, ref.shift, dH))
        SEEN["partials_scale"] = max(SEEN["partials_scale"], float(((sc.double() - ref.scale).abs() / (M.U32 * ref.scale.abs())).max()))


@pytest.mark.parametrize("types", M.LN_TYPES, ids=["%s-%s" % (M.DT_ID[a], M.DT_ID[b]) for a, b in M.LN_TYPES])
@pytest.mark.parametrize("i", range(len(M.LN_CASES)), ids=LN_IDS)
def test_layernorm_emulation_within_bounds(i, types):
    tin, tout = types
    SEEN["runs"] += 1
    for with_pe in (True, False):
        c, x, ref = M.ln_ref(i, tin, with_pe)
        bound = M.ln_bound(ref, x.gamma, tout, c.L)
        for fma in (False, True):
            y = M.emulate_layernorm(x.x, x.pe if with_pe else None, x.gamma, x.beta, tout, fma)
            r = M.assert_within("%s pe%d fma%d" % (c.name, with_pe, fma), y, ref.y, bound)
            SEEN["layernorm"] = max(SEEN["layernorm"], r)


def test_recorded_model_maxima():
    """The maxima in norm_model's docstring are what the emulation gives (re-measured here when the tests above were deselected),
    and the caps are twice them."""
    if SEEN["runs"] < N_RUNS:
        for i in range(len(M.GN_CASES)):
            for dtype in M.ALL3:
                test_groupnorm_emulation_within_bounds(i, dtype)
        for i in range(len(M.PART_CASES)):
            test_partials_emulation_within_bounds(i)
        for i in range(len(M.LN_CASES)):
            for types in M.LN_TYPES:
                test_layernorm_emulation_within_bounds(i, types)
    print("emulation maxima:", SEEN)
    for key, rec in M.MODEL_MAX.items():
        assert SEEN[key] <= rec * 1.001 and SEEN[key] >= rec * 0.95, (key, SEEN[key], rec)
    for arm, cap in M.CAP.items():
        assert abs(cap - 2 * M.MODEL_MAX[arm]) < 0.01
    assert M.MODEL_MAX["partials_scale"] <= 2 and M.MODEL_MAX["partials_shift"] < 1 and M.MODEL_MAX["layernorm"] < 1


def test_exact_rstd_interval_is_the_first_order_form_where_that_is_valid():
    seen = 0
    for i in range(len(M.GN_CASES)):
        c, x, ref = M.gn_ref(i, torch.float32)
        exact, first = M.rstd_interval(ref, c.L), M.rstd_first_order(ref, c.L)
        ok = 3 * c.L * M.U32 * ref.kappa < 1e-3
        seen += int(ok.sum())
        assert float((exact[ok] / first[ok] - 1).abs().max()) < 1e-3, c.name
        assert bool((exact >= first * (1 - 1e-9))[~ok & (3 * c.L * M.U32 * ref.kappa < 0.5)].all()), c.name
    assert seen > 100


# ------------------------------------------------------------------------------------------------ seeded defects
def _case(name):
    return next(c for c in M.GN_CASES if c.name == name)


GN_DEFECTS = (("the last pixel of a ragged chunk dropped", "drop_last_pixel", "two_stage-1x4099x320-g32"),
              ("the wrap weight applied to col <= wrap", "wrap_le", "two_stage-1x8580x320-g32-wrap132x2"),
              ("hw used for hw_counted", "hw_counted", "direct-2x96x64+32-g32-wrap16x2"),
              ("the second source read at channel offset c", "src_offset", "direct-3x408x64+32-g32"),
              ("one chunk's partial counted twice", "chunk_twice", "two_stage-1x4099x320-g32"))
LN_DEFECTS = (("one-pass LayerNorm variance on the offset rows", "one_pass"), ("positional encoding taken at row % (pe_rows + 1)", "pe_mod"),
              ("the last row of a 4-row group skipped", "skip_last_row"))
LN_DEFECT_CASE = "rows4-4099x320"
MUST_PASS_REL_L2 = ("drop_last_pixel", "src_offset", "chunk_twice")


def gn_flagged(c, x, ref, sc, sh):
    try:
        gn_check("defect", sc, sh, ref, c, x)
    except AssertionError:
        return True
    return False


@functools.lru_cache(maxsize=None)
def gn_defect(dtype, key, case_name, plain):
    """(flagged by the new checks, rel-L2 of the 16-bit GroupNorm + SiLU output against float64) of a seeded defect; plain: on
    the inputs of the suite's rel-L2 tests (kappa ~ 1), else on the ladder inputs of the case."""
    c = _case(case_name)
    x = M.plain_inputs(c, dtype, seed=7) if plain else M.gn_inputs(c, dtype, seed=7)
    ref = M.gn_reference(x.x, c.groups, x.gamma, x.beta, c.wrap)
    clean = M.emulate_groupnorm(x.x.float(), c.groups, x.gamma, x.beta, c.wrap)
    assert not gn_flagged(c, x, ref, *clean), "the clean emulation must pass"
    xx = M.concat_sources(x.x0, x.x1, key)
    sc, sh = M.emulate_groupnorm(xx, c.groups, x.gamma, x.beta, c.wrap, defect=key)
    y = M.apply_reference(x.x, sc, sh, 1).to(dtype)
    return gn_flagged(c, x, ref, sc, sh), rel_l2(y, M.apply_reference(x.x, ref.scale, ref.shift, 1))


@functools.lru_cache(maxsize=None)
def ln_defect(dtype, key):
    i = LN_IDS.index(LN_DEFECT_CASE)
    c, x, ref = M.ln_ref(i, dtype, True)
    bound = M.ln_bound(ref, x.gamma, dtype, c.L)
    y = M.emulate_layernorm(x.x, x.pe, x.gamma, x.beta, dtype, defect=key)
    try:
        M.assert_within("defect", y, ref.y, bound)
        flagged = False
    except AssertionError:
        flagged = True
    return flagged, rel_l2(y, ref.y)


@pytest.mark.parametrize("dtype", M.F16S, ids=["bf16", "fp16"])
def test_seeded_defects_are_flagged(dtype):
    for what, key, case_name in GN_DEFECTS:
        for plain in (True, False):
            flagged, err = gn_defect(dtype, key, case_name, plain)
            print("defect %-50s %-4s %-6s inputs: flagged %s" % (what, M.DT_ID[dtype], "plain" if plain else "ladder", flagged))
            assert flagged, "defect not flagged: %s (%s inputs)" % (what, "plain" if plain else "ladder")
    for what, key in LN_DEFECTS:
        flagged, err = ln_defect(dtype, key)
        print("defect %-50s %-4s flagged %s" % (what, M.DT_ID[dtype], flagged))
        assert flagged, "defect not flagged: " + what


def test_rel_l2_accepts_local_defects():
    """The gap this closes.  Every defect on the suite's own kind of input (randn * 2 + 0.5): would the rel-L2 tolerance of
    test_gpu_kernels.py have accepted the GroupNorm + SiLU / LayerNorm output?  The dropped pixel passes it in both types
    (rel-L2 1.7e-3 / 3.2e-4); in bf16 so do the second source read at the wrong offset (2.7e-3), the chunk counted twice (3.7e-3) and the
    one-pass variance (1.7e-3).  The wrap weight on one column too many does NOT at width 132 (5.9e-3 against 4e-3: the column's
    mass is added, not re-weighted), nor does hw for hw_counted (0.16): printed with the rest, not asserted."""
    accepted = {}
    for dtype in M.F16S:
        for what, key, case_name in GN_DEFECTS:
            flagged, err = gn_defect(dtype, key, case_name, True)
            ok = err <= M.OLD_TOL[dtype]
            accepted[(key, dtype)] = ok
            print("rel-L2 %-50s %-4s %.3e (TOL %.1e): %s" % (what, M.DT_ID[dtype], err, M.OLD_TOL[dtype], "ACCEPTED" if ok else "rejected"))
        for what, key in LN_DEFECTS:
            flagged, err = ln_defect(dtype, key)
            ok = err <= M.OLD_TOL[dtype]
            print("rel-L2 %-50s %-4s %.3e (TOL %.1e): %s" % (what, M.DT_ID[dtype], err, M.OLD_TOL[dtype], "ACCEPTED" if ok else "rejected"))
    assert all(accepted[("drop_last_pixel", dtype)] for dtype in M.F16S)
    for key in MUST_PASS_REL_L2:
        assert accepted[(key, torch.bfloat16)], key


def _dropped_pixel(name, pix):
    """(bound / effect, (cap + final roundings) / effect) on rstd per (image, group) with kappa <= 10: effect = what zeroing pixel
    `pix` does to rstd, exactly, in float64."""
    c, x, ref = M.gn_ref(GN_IDS.index(name), torch.float32)
    xd = x.x.clone()
    xd[:, pix] = 0
    hit = M.gn_reference(xd, c.groups, x.gamma, x.beta)
    effect = (hit.rstd / ref.rstd - 1).abs()
    sel = ref.kappa <= 10
    assert int(sel.sum()) >= 8
    return (M.rstd_interval(ref, c.L) / effect)[sel], ((M.CAP[c.arm] * ref.kappa + 2) * M.U32 / effect)[sel]


def test_hard_bound_is_not_hollow():
    """The case with the most pixels per group (16411 x 2, L = 67), groups with kappa <= 10: the hard bound on rstd is a fifth of
    what ONE dropped pixel does to rstd (median over the groups) and below it in at least three groups of four (a pixel whose
    squares happen to equal the group's mean square moves nothing).  The cap is below the effect in EVERY such group of every
    two-stage case -- including the one with L = 513 (pix_par = 128 slots walked serially), where the hard bound only equals
    the effect (median 0.9): there the cap alone separates a dropped pixel from rounding."""
    name = "two_stage-1x16411x64-g32"
    assert _case(name).hw == max(k.hw for k in M.GN_CASES)
    for pix in (16409, 8205, 7):                         # (16410, the last pixel, carries an outlier: its effect is far larger)
        hard, cap = _dropped_pixel(name, pix)
        print("dropped pixel %5d of %s: bound / effect median %.2f max %.2f, below 1 in %.0f %%; cap / effect max %.3f"
              % (pix, name, float(hard.median()), float(hard.max()), 100 * float((hard < 1).double().mean()), float(cap.max())))
        assert float(hard.median()) < 0.5 and float((hard < 1).double().mean()) >= 0.75
    for c in M.GN_CASES:
        if c.arm == "two_stage" and c.wrap is None:
            hard, cap = _dropped_pixel(c.name, c.hw // 2)
            print("dropped pixel of %-40s L %3d: bound / effect median %.2f; cap / effect max %.3f" % (c.name, c.L, float(hard.median()), float(cap.max())))
            assert float(cap.max()) < 1, c.name
