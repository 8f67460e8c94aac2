"""Cases, rounding-model configuration and row cap of the wide-head flash attention (pf_attention_wide, D in {128, 256, 512}).
A helper module: no tests in it.  Everything numerical comes from tests/attention_model.py: the float64 reference, the
componentwise bound |got - O| <= 4 u A + F and the per-row RMS statistic apply unchanged at these widths
(test_attention_wide_cpu.py::test_model_maxima re-measures the model at the configuration the kernel uses).

The kernel's rounding points (header comment of pf_attention_wide.hip): key tiles of 64, the softmax reference point moved at
every tile (no deferred rescale), P rounded to the 16-bit type before the second product, the denominator from the UNROUNDED
P in fp32 (not the MSUM form).

Model maxima at that configuration over WIDE_CASES, both types, fp16 subnormals of P kept and flushed:
    max |err| / (4 u A + F)   0.191
    max row RMS               0.167  ->  ROW_CAP_WIDE = 0.34 (twice the model's largest row RMS, rounded up)
    max median F / (u A)      0.062  (staircase, fp16; the project's rule is < 0.1)
"""
import functools

import attention_model as M

# (msum, tile, defer) of emulate_forward that states what k_attention_wide does
KERNEL_MODEL = dict(msum=False, tile=64, defer=0.0)

WIDE_CASES = [
    M.make_case("wide", 1, 1, 512, 33, 1),                                  # one key, ragged query tile
    M.make_case("wide", 2, 1, 512, 100, 77),                                # ragged on both sides, batch strides
    M.make_case("wide", 1, 1, 512, 130, 192),
    M.make_case("wide", 1, 1, 512, 64, 448, variant="staircase"),           # the rescale path across key tiles
    M.make_case("wide", 1, 1, 512, 64, 448, variant="spike"),
    M.make_case("wide", 2, 1, 512, 96, 1100),                               # many key tiles, ragged last tile
    M.make_case("wide", 1, 2, 256, 70, 200),
    M.make_case("wide", 1, 1, 128, 70, 200),
]

MODEL_MAX_WIDE = dict(ELEM=0.191, ROW=0.167, F_MEDIAN=0.062)
ROW_CAP_WIDE = 0.34


@functools.lru_cache(maxsize=None)
def wide_ref(i, dtype):
    """(case, inputs, float64 reference) of WIDE_CASES[i], computed once per process and shared by the test modules."""
    c = WIDE_CASES[i]
    x = M.make_inputs(c, dtype, seed=200 + i)
    return c, x, M.ref_forward(x.q, x.k, x.v, c.H, x.scale)
