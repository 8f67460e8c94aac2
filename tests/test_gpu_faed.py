"""The FAED metric on the GPU: pf_pano_conv per encoder arm against the float64 layer model with a per-element bound, periodicity bit
for bit, pf_faed_features, the seeded encoder end to end on the fixture, and the metric's states."""
import os

import numpy as np
import pytest
import torch

import faed_model as FM
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32, U16 = 2.0 ** -24, 2.0 ** -11          # unit round-offs of fp32 and fp16

# (ksize, stride, c_in, n_out) of the encoder; c_in 3 is the image layer
ARMS = [(9, 1, 3, 32), (9, 1, 32, 32), (4, 2, 32, 64), (7, 1, 64, 64), (4, 2, 64, 128), (5, 1, 128, 128), (4, 2, 128, 128), (3, 1, 128, 128)]
SHAPES = {1: [(3, 6), (7, 20), (16, 36)], 2: [(2, 2), (6, 12), (8, 40)]}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "faed.npz"))


def _problem(k, s, ci, co, h, w, seed, float_image=False):
    """Seeded operands of one layer, n = 2: (device x, fp16 NHWC operand as numpy, w16, scale, shift, residual16)."""
    rng = np.random.default_rng(seed)
    n = 2
    if ci == 3:
        imgs = rng.uniform(0, 255, (n, 3, h, w)).astype(np.float32) if float_image else rng.integers(0, 256, (n, 3, h, w)).astype(np.uint8)
        x_dev, x16 = torch.from_numpy(imgs).to(DEV), FM.image_operand(imgs)
    else:
        x16 = rng.normal(0, 1, (n, h, w, ci)).astype(np.float16)
        x_dev = torch.from_numpy(x16).to(DEV)
    w16 = (rng.normal(0, 1, (co, k, k, ci)) / np.sqrt(k * k * ci)).astype(np.float16)
    scale, shift = rng.uniform(0.5, 1.5, co).astype(np.float32) * rng.choice([-1.0, 1.0], co).astype(np.float32), rng.normal(0, 0.3, co).astype(np.float32)
    p = FM.pad_of(k, s)
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    res16 = rng.normal(0, 1, (n, ho, wo, co)).astype(np.float16)
    return x_dev, x16, w16, scale, shift, res16


def _run(x_dev, w16, scale, shift, k, s, relu, res16, out32):
    from panfusion_amd import ops
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    out = ops.pano_conv(x_dev, t(w16), t(scale), t(shift), k, s, relu=relu, residual=t(res16), out_dtype=torch.float32 if out32 else torch.float16)
    return out.double().cpu().numpy()


@pytest.mark.parametrize("arm", ARMS, ids=lambda a: "k%ds%d_%dto%d" % a)
def test_layer_within_summation_bound(arm):
    """Every element within (K + 4) 2^-24 (sum |a w| |scale| + |shift| + |residual|) + 2^-11 |exact| of the float64 layer on the same
    fp16 operands (the last term only for fp16 output): the worst-case fp32 summation in any order plus one output rounding.  n = 2:
    a row of the neighbouring image read as padding would show."""
    k, s, ci, co = arm
    shapes = list(SHAPES[s]) + ([(5, 4)] if (k, s) == (9, 1) else [])          # w == pad
    worst = 0.0
    for h, w in shapes:
        for float_image in ([False, True] if ci == 3 else [False]):
            x_dev, x16, w16, scale, shift, res16 = _problem(k, s, ci, co, h, w, 100 * h + w, float_image)
            for relu in (False, True):
                for use_res in (False, True):
                    for out32 in (False, True):
                        r = res16 if use_res else None
                        exact, mag = FM.conv_layer(x16, w16, k, s, scale, shift, relu, r)
                        got = _run(x_dev, w16, scale, shift, k, s, relu, r, out32)
                        assert got.shape == exact.shape
                        bound = (k * k * ci + 4) * U32 * mag + (0.0 if out32 else U16 * np.abs(exact))
                        share = float((np.abs(got - exact) / bound).max())
                        worst = max(worst, share)
                        assert share <= 1.0, (arm, (h, w), relu, use_res, out32, share)
    print("arm %s: largest share of the bound %.3f" % (arm, worst))


def _forced_rows(rows, fn):
    """fn() with PF_PANO_CONV_ROWS = rows, or unset for None (the library reads it at every call)."""
    old = os.environ.pop("PF_PANO_CONV_ROWS", None)
    if rows is not None:
        os.environ["PF_PANO_CONV_ROWS"] = str(rows)
    try:
        return fn()
    finally:
        os.environ.pop("PF_PANO_CONV_ROWS", None)
        if old is not None:
            os.environ["PF_PANO_CONV_ROWS"] = old


@pytest.mark.parametrize("arm", [a for a in ARMS if a[0] in (5, 7, 9) and a[2] != 3], ids=lambda a: "k%ds%d_%dto%d" % a)
def test_sixteen_row_tiles_within_bound_and_same_bits(arm):
    """The stride-1 kernel's second form (16 x 16 tiles, 4 rows per wavefront; the 5-, 7- and 9-wide kernels have it), forced at a
    small size with rows that are no multiple of 16 and more than one tile: inside the same bound, and bit for bit the 8-row form's
    result.  pf_pano_conv_tile_rows says which form each call ran."""
    from panfusion_amd import ops
    k, s, ci, co = arm
    h, w = 19, 36
    x_dev, x16, w16, scale, shift, res16 = _problem(k, s, ci, co, h, w, 11 * k + ci)
    exact, mag = FM.conv_layer(x16, w16, k, s, scale, shift, True, res16)
    bound = (k * k * ci + 4) * U32 * mag + U16 * np.abs(exact)
    run = lambda: (ops.pano_conv_tile_rows(k, s, 2, h, w), _run(x_dev, w16, scale, shift, k, s, True, res16, False))
    rows16, sixteen = _forced_rows(4, run)
    rows8, eight = _forced_rows(2, run)
    assert (rows16, rows8) == (16, 8)
    assert float((np.abs(sixteen - exact) / bound).max()) <= 1.0
    assert np.array_equal(sixteen, eight)


def test_sixteen_row_tiles_chosen_at_512_tiles_keep_bits():
    """2 x 256 x 256 is exactly 512 tiles of 16 x 16, where the library itself takes the 16-row form (pf_pano_conv_tile_rows says so;
    test_faed_cpu.py pins the threshold from both sides): the 9 x 9 32 -> 32 layer there is inside the bound and equals the forced
    8-row form bit for bit."""
    from panfusion_amd import ops
    k, s, ci, co = 9, 1, 32, 32
    x_dev, x16, w16, scale, shift, res16 = _problem(k, s, ci, co, 256, 256, 5)
    exact, mag = FM.conv_layer(x16, w16, k, s, scale, shift, False, None)
    bound = (k * k * ci + 4) * U32 * mag + U16 * np.abs(exact)
    rows, auto = _forced_rows(None, lambda: (ops.pano_conv_tile_rows(k, s, 2, 256, 256), _run(x_dev, w16, scale, shift, k, s, False, None, False)))
    assert rows == 16
    eight = _forced_rows(2, lambda: _run(x_dev, w16, scale, shift, k, s, False, None, False))
    assert float((np.abs(auto - exact) / bound).max()) <= 1.0
    assert np.array_equal(auto, eight)


@pytest.mark.parametrize("arm", ARMS, ids=lambda a: "k%ds%d_%dto%d" % a)
@pytest.mark.parametrize("w", [20, 36])
def test_periodicity_bit_for_bit(arm, w):
    """Rolling the input by r columns rolls the output by r (stride 1) or r / 2 (stride 2, even r) with identical bits: r = 1, pad and
    w - 1 at stride 1; at stride 2, where an odd shift has no image, twice those."""
    k, s, ci, co = arm
    p = FM.pad_of(k, s)
    h = 8
    x_dev, x16, w16, scale, shift, res16 = _problem(k, s, ci, co, h, w, 7 * w + k)
    base = _run(x_dev, w16, scale, shift, k, s, True, None, False)
    wdim = 3 if ci == 3 else 2
    for r in ((1, p, w - 1) if s == 1 else (2, 2 * p + 2, w - 2)):
        got = _run(torch.roll(x_dev, r, dims=wdim), w16, scale, shift, k, s, True, None, False)
        assert np.array_equal(got, np.roll(base, r // s, axis=2)), (arm, w, r)


@pytest.mark.parametrize("shape", [(2, 5, 6, 128), (1, 3, 14, 128), (3, 16, 32, 128)])
def test_features_within_bound(shape):
    from panfusion_amd import ops
    n, hp, wp, c = shape
    g = torch.Generator().manual_seed(hp)
    x = torch.randn(shape, generator=g) + 0.5
    weight = torch.cos(torch.linspace(np.pi / 2, -np.pi / 2, hp))
    got = ops.faed_features(x.to(DEV), weight.to(DEV)).double().cpu().numpy()
    want = FM.features_of(x.double().numpy(), weight.double().numpy())
    mean_abs = np.transpose(np.abs(x.double().numpy()).mean(axis=2), (0, 2, 1)).reshape(n, c * hp)
    wrow = np.tile(np.abs(weight.double().numpy()), c)[None]
    bound = (wp + 2) * U32 * mean_abs * wrow
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())


@pytest.fixture(scope="module")
def encoder(fixture):
    from panfusion_amd.models.faed import Encoder
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(int(fixture["seed"])).items()}
    return Encoder.from_state_dict(sd, device=DEV, max_batch=2)


@pytest.mark.parametrize("case", ["a", "b"])
def test_encoder_end_to_end(fixture, encoder, case):
    """Feature rel-L2 against the reference's float64 features <= 1e-3 (the project's gate for fp16 operands)."""
    imgs, want = torch.from_numpy(fixture["imgs_" + case]), fixture["features_" + case]
    got = encoder.features(imgs).double().cpu().numpy()
    rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print("case %s: feature rel-L2 against float64 %.3e" % (case, rel))
    assert got.shape == want.shape and rel <= 1e-3, rel
    f32 = encoder.features(imgs.float()).double().cpu().numpy()              # the float form of the same images
    assert np.array_equal(f32, got)


def test_batch_chunking_keeps_bits(fixture, encoder):
    from panfusion_amd.models.faed import Encoder
    imgs = torch.from_numpy(fixture["imgs_a"])
    two = encoder.features(imgs)
    one = Encoder(encoder.layers, DEV, max_batch=1)
    assert torch.equal(one.features(imgs), two)
    assert torch.equal(one(imgs), encoder(imgs))


def test_metric_states_and_compute(fixture, encoder):
    """update() with case A as the real side and a seeded perturbation of it as the generated side: exact counts, the float64 sums
    within 2e-3 |f| and the f^T f sums within 4e-3 |f|^2 of the model's states (what the 1e-3 feature gate implies), and compute()
    on the device equal to compute() on the same states on the host.  The Fréchet value itself is not gated at this size: with two
    samples per side the covariances are singular and the value is ill-conditioned."""
    from panfusion_amd.models.faed import FrechetAutoEncoderDistance
    from panfusion_amd.pipeline import faed
    real = torch.from_numpy(fixture["imgs_a"])
    fake = torch.from_numpy(FM.perturb(fixture["imgs_a"], int(fixture["seed"])))
    m = FrechetAutoEncoderDistance(real.shape[2], encoder)
    value = faed(real, fake, m)
    assert m.real_features_sum.is_cuda and m.real_features_cov_sum.dtype == torch.float64
    assert int(m.real_features_num_samples) == 2 and int(m.fake_features_num_samples) == 2
    for side, f in (("real", fixture["features_a"]), ("fake", fixture["features_fake_a"])):
        s, c, n = FM.states(f)
        norm = np.linalg.norm(f)
        ds = np.linalg.norm(getattr(m, side + "_features_sum").cpu().numpy() - s)
        dc = np.linalg.norm(getattr(m, side + "_features_cov_sum").cpu().numpy() - c)
        print("%s: sum error %.2e |f|, f^T f error %.2e |f|^2" % (side, ds / norm, dc / norm ** 2))
        assert ds <= 2e-3 * norm and dc <= 4e-3 * norm ** 2
    host = FrechetAutoEncoderDistance(real.shape[2]).merge(m)
    assert not host.real_features_sum.is_cuda
    want = float(host.compute())
    print("FAED (2 + 2 samples, not gated): %.6f on the device, %.6f on the host" % (float(value), want))
    assert value.is_cuda and abs(float(value) - want) <= 1e-9 * abs(want)
    m.reset()
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()
