"""The per-element and per-row attention checks of tests/attention_model.py, exercised without a GPU: the rounding model
of the kernels stays inside them on every case of tests/test_gpu_attention_bounds.py, seeded local defects are flagged
(most of which the suite's rel-L2 tolerance accepts), and the fp16 underflow term does not hollow the bounds."""
import functools

import pytest
import torch

import attention_model as M
from conftest import rel_l2

DTYPES = [torch.bfloat16, torch.float16]
FLUSHES = {torch.bfloat16: (False,), torch.float16: (False, True)}
BWD = (("dq", "dQ", "A_Q", "F_Q"), ("dk", "dK", "A_K", "F_K"), ("dv", "dV", "A_V", "F_V"))
SEEN = dict(FWD_ELEM=0.0, BWD_ELEM=0.0, FWD_ROW=0.0, BWD_ROW=0.0, runs=0)      # filled by the two model tests below


fwd_ref, bwd_ref = M.fwd_ref, M.bwd_ref


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(M.FWD_CASES)), ids=[c.name for c in M.FWD_CASES])
def test_forward_model_within_bounds(i, dtype):
    c, x, ref = fwd_ref(i, dtype)
    bound = M.forward_bound(ref, dtype)
    SEEN["runs"] += 1
    for (msum, S, tile, defer) in M.model_configs(c):
        for flush in FLUSHES[dtype]:
            out, lse = M.emulate_forward(x.q, x.k, x.v, c.H, x.scale, x.bias, dtype=dtype, msum=msum, splits=S, flush=flush, tile=tile, defer=defer)
            name = "%s msum%d S%d flush%d" % (c.name, msum, S, flush)
            M.assert_within(name, out, ref.O, bound, c.H)
            SEEN["FWD_ROW"] = max(SEEN["FWD_ROW"], M.assert_rows(name, out, ref.O, ref.A, c.H, dtype, M.ROW_CAP_FWD, ref.F))
            if not flush:
                SEEN["FWD_ELEM"] = max(SEEN["FWD_ELEM"], M.worst_ratio(out, ref.O, M.U[dtype] * ref.A))
            if c.lse:                                   # (requested only from arms that keep fp32 row sums)
                assert float((lse.double() - ref.lse).abs().max()) < 2e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("i", range(len(M.BWD_CASES)), ids=[c.name for c in M.BWD_CASES])
def test_backward_model_within_bounds(i, dtype):
    c, x, ref = bwd_ref(i, dtype)
    bounds = M.backward_bounds(ref, dtype)
    SEEN["runs"] += 1
    for flush in FLUSHES[dtype]:
        got = M.emulate_backward(x.q, x.k, x.v, x.dout, ref.lse.float(), ref.delta.float(), c.H, x.scale, x.bias, dtype=dtype, flush=flush)
        for n, R, A, F in BWD:
            name = "%s %s flush%d" % (c.name, n, flush)
            M.assert_within(name, got[n], getattr(ref, R), bounds[n], c.H)
            SEEN["BWD_ROW"] = max(SEEN["BWD_ROW"], M.assert_rows(name, got[n], getattr(ref, R), getattr(ref, A), c.H, dtype, M.ROW_CAP_BWD, getattr(ref, F)))
            if not flush:
                SEEN["BWD_ELEM"] = max(SEEN["BWD_ELEM"], M.worst_ratio(got[n], getattr(ref, R), M.U[dtype] * getattr(ref, A)))


def test_recorded_model_maxima():
    """The maxima written into attention_model's docstring are what the model gives (this runs after the two tests above and
    re-measures when they were deselected): the row caps are twice them, the componentwise maxima sit well below 4 and 3."""
    if SEEN["runs"] < 2 * (len(M.FWD_CASES) + len(M.BWD_CASES)):
        for dtype in DTYPES:
            for i in range(len(M.FWD_CASES)):
                test_forward_model_within_bounds(i, dtype)
            for i in range(len(M.BWD_CASES)):
                test_backward_model_within_bounds(i, dtype)
    print("model maxima:", SEEN)
    for key, rec in M.MODEL_MAX.items():
        assert SEEN[key] <= rec * 1.001 and SEEN[key] >= rec * 0.95, (key, SEEN[key], rec)
    assert abs(M.ROW_CAP_FWD - 2 * M.MODEL_MAX["FWD_ROW"]) < 0.01 and abs(M.ROW_CAP_BWD - 2 * M.MODEL_MAX["BWD_ROW"]) < 0.01
    assert M.MODEL_MAX["FWD_ELEM"] < 2 and M.MODEL_MAX["BWD_ELEM"] < 1.5


@pytest.mark.parametrize("i", range(len(M.FWD_CASES)), ids=[c.name for c in M.FWD_CASES])
def test_fp16_underflow_term_does_not_hollow_the_forward_bound(i):
    c, x, ref = fwd_ref(i, torch.float16)
    assert float((ref.F / (M.U[torch.float16] * ref.A)).median()) < 0.1


@pytest.mark.parametrize("i", range(len(M.BWD_CASES)), ids=[c.name for c in M.BWD_CASES])
def test_fp16_underflow_term_does_not_hollow_the_backward_bounds(i):
    c, x, ref = bwd_ref(i, torch.float16)
    for n, R, A, F in BWD:
        assert float((getattr(ref, F) / (M.U[torch.float16] * getattr(ref, A))).median()) < 0.1, n


# ------------------------------------------------------------------------------------------------ seeded defects
DEFECTS = ("padded key joins", "bias dropped in the last query tile", "last row duplicated", "split drops its last tile", "row scaled by 1.1")
# 65536 query rows (one garbage row moves the rel-L2 by sqrt(2 / 65536) = 5.5e-3); scores of standard deviation 2 (a softmax whose rows have a few dominant keys, as the EPA attention has:
# with a flat softmax O is a small difference of large terms and no bound made of magnitudes can see 10 % of it)
DEFECT_CASE = M.make_case("d32split", 8, 1, 32, 8192, 128, bias=True, S=2, qscale=2.0)
TILE = 32                              # key tile of the model here: two splits of two tiles
CANARY = 1000.0


@functools.lru_cache(maxsize=1)
def defect_outputs(dtype):
    c = DEFECT_CASE
    x = M.make_inputs(c, dtype, seed=77)
    x.bias[-32:, :32] = torch.rand(32, 32, generator=torch.Generator().manual_seed(5)) * 2       # the last query tile has a bias for sure
    x.bias *= 0.15                                          # (a mild bias, at most 0.3: losing it is a small error)
    ref = M.ref_forward(x.q, x.k, x.v, c.H, x.scale, x.bias)
    run = lambda k, v, bias: M.emulate_forward(x.q, k, v, c.H, x.scale, bias, dtype=dtype, splits=c.S, tile=TILE)[0]
    clean = run(x.k, x.v, x.bias)
    out = {}
    # a padded key joins the softmax: score 0 (a zero K row), V canary
    k1 = torch.cat([x.k, torch.zeros(c.B, 1, c.H * c.D, dtype=dtype)], 1)
    v1 = torch.cat([x.v, torch.full((c.B, 1, c.H * c.D), CANARY, dtype=dtype)], 1)
    out[DEFECTS[0]] = M.emulate_forward(x.q, k1, v1, c.H, x.scale, torch.cat([x.bias, torch.zeros(c.nq, 1)], 1), dtype=dtype, tile=TILE)[0]
    # the bias flag is lost for the last 32-row query tile only
    nobias = x.bias.clone()
    nobias[-32:] = 0
    d = clean.clone()
    d[:, -32:] = run(x.k, x.v, nobias)[:, -32:]
    out[DEFECTS[1]] = d
    d = clean.clone()
    d[-1, -1] = d[-1, -2]
    out[DEFECTS[2]] = d
    # the first split skips its last key tile (keys 32..63 get no weight)
    skip = x.bias.clone()
    skip[:, TILE:2 * TILE] = float("-inf")
    out[DEFECTS[3]] = run(x.k, x.v, skip)
    d = clean.clone()
    d[1, 4321] = (d[1, 4321] * 1.1).to(dtype).float()
    out[DEFECTS[4]] = d
    return c, ref, clean, out


def new_checks_pass(c, ref, got, dtype):
    try:
        M.assert_within("defect", got, ref.O, M.forward_bound(ref, dtype), c.H)
        M.assert_rows("defect", got, ref.O, ref.A, c.H, dtype, M.ROW_CAP_FWD, ref.F)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_seeded_defects_are_flagged(dtype):
    c, ref, clean, out = defect_outputs(dtype)
    assert new_checks_pass(c, ref, clean, dtype), "the clean model output must pass"
    for name in DEFECTS:
        assert not new_checks_pass(c, ref, out[name], dtype), "defect not flagged: " + name


def test_rel_l2_accepts_most_of_the_defects():
    """The gap this closes: the suite's rel-L2 <= 2.5 TOL accepts at least three of the five defects in at least one type."""
    accepted = set()
    for dtype in DTYPES:
        c, ref, clean, out = defect_outputs(dtype)
        for name in DEFECTS:
            err = rel_l2(out[name], ref.O)
            print("%-40s %s rel-L2 %.3e (tolerance %.1e)" % (name, dtype, err, M.OLD_TOL[dtype]))
            if torch.isfinite(out[name]).all() and err <= M.OLD_TOL[dtype]:
                accepted.add(name)
    assert len(accepted) >= 3, sorted(accepted)
