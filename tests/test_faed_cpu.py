"""The FAED metric without a GPU: the float64 model against the reference's recorded features, the Fréchet distance against its
matrix-square-root form, the metric class on given states, BatchNorm folding, and the host side of pf_pano_conv."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import faed_model as FM
from conftest import GOLDEN, ROOT
from panfusion_amd import _lib
from panfusion_amd.models.faed import FrechetAutoEncoderDistance
from panfusion_amd.models.faed import modules as M


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "faed.npz"))


def test_model_reproduces_reference_features(fixture):
    sd = FM.state_dict(int(fixture["seed"]))
    for case in "ab":
        got = FM.features(sd, fixture["imgs_" + case])
        err = np.abs(got - fixture["features_" + case]).max()
        print("case %s: model vs recorded reference features %.2e" % (case, err))
        assert err <= 1e-9


def test_fixture_covers_what_it_is_for(fixture):
    a, b = fixture["imgs_a"], fixture["imgs_b"]
    assert a.dtype == np.uint8 and a.shape == (2, 3, 160, 192) and b.shape == (1, 3, 96, 448)
    assert a.shape[2] // 32 == 5 and b.shape[3] // 32 == 14                       # h' = 5 (weights 0, .71, 1, .71, 0), w' = 14
    assert fixture["features_a"].shape == (2, 640) and fixture["features_b"].shape == (1, 384)
    assert np.allclose(FM.latitude_weight(5), [0, np.sqrt(0.5), 1, np.sqrt(0.5), 0], atol=1e-15)
    assert float(fixture["e32_a"]) < 1e-6 and float(fixture["e32_b"]) < 1e-6
    # the features depend on the image, not on the biases alone
    assert np.abs(fixture["features_a"][0] - fixture["features_a"][1]).max() > 1e-3
    assert len(FM.state_dict(0)) == 109 and sorted(FM.state_dict(0)) == sorted(M.expected_keys())


def _sqrtm_form(f1, f2):
    from scipy.linalg import sqrtm
    m1, m2 = f1.mean(0), f2.mean(0)
    c1, c2 = np.cov(f1, rowvar=False), np.cov(f2, rowvar=False)
    return float(((m1 - m2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(sqrtm(c1 @ c2)).real)


def _synthetic(n, d, seed):
    rng = np.random.default_rng(seed)
    mix = np.eye(d) + 0.3 * rng.normal(size=(d, d)) / np.sqrt(d)
    return rng.normal(size=(n, d)) @ mix + rng.normal(size=d)


@pytest.mark.parametrize("d", [32, 48])
def test_frechet_equals_sqrtm_form(d):
    f1, f2 = _synthetic(4 * d, d, d), _synthetic(4 * d + 3, d, d + 1)
    got, want = FM.frechet(f1, f2), _sqrtm_form(f1, f2)
    print("d %d: eigenvalue form %.12f, sqrtm form %.12f, rel %.1e" % (d, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-9 * abs(want)


def test_frechet_singular_case():
    """n = 20 < d: the covariances are singular and the root of the near-zero eigenvalues is ill-conditioned: 1e-7."""
    f1, f2 = _synthetic(20, 32, 5), _synthetic(20, 32, 6)
    got, want = FM.frechet(f1, f2), _sqrtm_form(f1, f2)
    print("singular: rel %.1e" % (abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-7 * abs(want)


def _metric_from(f1, f2):
    m = FrechetAutoEncoderDistance(f1.shape[1] // 4)
    for side, f in (("real", f1), ("fake", f2)):
        s, c, n = FM.states(f)
        getattr(m, side + "_features_sum").copy_(torch.from_numpy(s))
        getattr(m, side + "_features_cov_sum").copy_(torch.from_numpy(c))
        getattr(m, side + "_features_num_samples").fill_(n)
    return m


def test_compute_equals_model_on_given_states():
    f1, f2 = _synthetic(130, 32, 1), _synthetic(150, 32, 2)
    got, want = float(_metric_from(f1, f2).compute()), FM.frechet(f1, f2)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


class _GivenFeatures:
    """Stands in for the encoder: the 'images' ARE the features."""
    device = torch.device("cpu")

    def features(self, imgs):
        return imgs[:, 0, 0, :].float()


def test_update_merge_reset_and_too_few_samples():
    f = torch.from_numpy(_synthetic(12, 8, 3)).float()
    g = torch.from_numpy(_synthetic(9, 8, 4)).float()
    as_imgs = lambda t: t[:, None, None, :]
    one = FrechetAutoEncoderDistance(2, _GivenFeatures())
    one.update(as_imgs(f), True)
    one.update(as_imgs(g), False)
    parts = [FrechetAutoEncoderDistance(2, _GivenFeatures()) for _ in range(2)]
    parts[0].update(as_imgs(f[:5]), True)
    parts[1].update(as_imgs(f[5:]), True)
    parts[0].update(as_imgs(g[:1]), False)
    parts[1].update(as_imgs(g[1:]), False)
    merged = parts[0].merge(parts[1])
    assert int(merged.real_features_num_samples) == 12 and int(merged.fake_features_num_samples) == 9
    assert merged.real_features_sum.dtype == torch.float64 and merged.real_features_cov_sum.shape == (8, 8)
    for name in ("real_features_sum", "real_features_cov_sum", "fake_features_sum", "fake_features_cov_sum"):
        a, b = getattr(merged, name), getattr(one, name)
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), name
    want = FM.frechet(f.double().numpy(), g.double().numpy())
    assert abs(float(merged.compute()) - want) <= 1e-9 * abs(want)
    assert abs(float(one.compute()) - want) <= 1e-9 * abs(want)
    one.reset()
    assert int(one.real_features_num_samples) == 0 and float(one.fake_features_cov_sum.abs().max()) == 0.0
    one.update(as_imgs(f), True)
    one.update(as_imgs(g[:1]), False)
    with pytest.raises(RuntimeError, match="More than one sample"):
        one.compute()
    with pytest.raises(RuntimeError, match="More than one sample"):
        FM.frechet(f.numpy(), g[:1].numpy())


def test_pipeline_faed_runs_both_sides():
    from panfusion_amd.pipeline import faed
    f = torch.from_numpy(_synthetic(12, 8, 3)).float()[:, None, None, :]
    g = torch.from_numpy(_synthetic(9, 8, 4)).float()[:, None, None, :]
    m = FrechetAutoEncoderDistance(2, _GivenFeatures())
    m.update(g, True)                                              # stale state: faed() resets
    got = float(faed([f[:4], f[4:]], g, m))
    want = FM.frechet(f[:, 0, 0].double().numpy(), g[:, 0, 0].double().numpy())
    assert abs(got - want) <= 1e-9 * abs(want)


def test_batchnorm_folding_equals_unfolded():
    sd = FM.state_dict(7)
    rng = np.random.default_rng(0)
    for L in FM.LAYERS:
        v = rng.normal(size=(50, L["co"])) * 3
        want = FM.unfolded(sd, L, v)
        t = lambda key: torch.from_numpy(np.asarray(sd[key]))
        bn = [t("%s.%s" % (L["norm"], p)) for p in ("weight", "bias", "running_mean", "running_var")] if L["norm"] else []
        scale, shift = M.fold_batchnorm(t(L["conv"] + ".bias"), *bn)
        got = v * scale.numpy() + shift.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), L["name"]
        ms, mh = FM.fold(sd, L)
        assert np.abs(ms - scale.numpy()).max() <= 1e-15 and np.abs(mh - shift.numpy()).max() <= 1e-15


def test_encoder_load_is_strict_and_inference_only():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(1).items()}
    enc = M.Encoder.from_state_dict(sd, device="cpu")
    assert len(enc.layers) == 17 and enc.layers[1][0].shape == (32, 9, 9, 32) and enc.layers[1][0].dtype == torch.float16
    prefixed = {"net.encoder." + k: v for k, v in sd.items()}
    prefixed["net.decoder.outconv_rgb.conv2d.bias"] = torch.zeros(3)         # the decoder is not the metric's
    enc2 = M.Encoder.from_state_dict(prefixed, device="cpu")
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) for a, b in zip(enc.layers, enc2.layers))
    with pytest.raises(KeyError, match="fuse.conv2d.bias"):
        M.Encoder.from_state_dict({k: v for k, v in sd.items() if k != "fuse.conv2d.bias"}, device="cpu")
    with pytest.raises(KeyError, match="surplus"):
        M.Encoder.from_state_dict(dict(sd, surplus=torch.zeros(1)), device="cpu")
    with pytest.raises(ValueError, match="shape"):
        M.Encoder.from_state_dict(dict(sd, **{"fuse.conv2d.bias": torch.zeros(64)}), device="cpu")
    with pytest.raises(RuntimeError, match="inference only"):
        enc.train()
    assert enc.train(False) is enc and enc.eval() is enc
    with pytest.raises(ValueError, match="multiples of 32"):
        enc(torch.zeros(1, 3, 48, 64, dtype=torch.uint8))
    assert M.flops_per_image(512, 1024) > 3.0e11


def test_pano_conv_desc_layout_matches_header(tmp_path):
    """_lib.PanoConvDesc against include/panfusion_hip.h through a gcc probe (as tests/test_abi.py pins the older structs)."""
    cname, cls = "pf_pano_conv_desc", _lib.PanoConvDesc
    lines = ['printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in cls._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "panfusion_hip.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        field, value = line.split()
        want = C.sizeof(cls) if field == "sizeof" else getattr(cls, field).offset
        assert int(value) == want, (field, value, want)
        seen += 1
    assert seen == len(cls._fields_) + 1
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "panfusion_hip.h")).read(), flags=re.S)
    end = hdr.index("} %s;" % cname)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    assert sorted(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|;)", body)) == sorted(f for f, _ in cls._fields_)


def _desc(**kw):
    """A valid 9 x 9 32 -> 32 problem on fake (never dereferenced) device addresses."""
    d = _lib.PanoConvDesc()
    d.x, d.weight, d.scale, d.shift, d.out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    d.x_dtype, d.out_dtype = _lib.PF_F16, _lib.PF_F16
    d.n_img, d.h, d.w, d.c_in, d.n_out, d.ksize, d.stride = 2, 16, 32, 32, 32, 9, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pano_conv_rejects_bad_arguments_before_any_launch():
    lib = _lib.lib()
    bad = [
        (dict(x=0), b"null pointer: x"), (dict(weight=0), b"null pointer: weight"), (dict(scale=0), b"null pointer: scale"),
        (dict(shift=0), b"null pointer: shift"), (dict(out=0), b"null pointer: out"),
        (dict(ksize=6), b"ksize"), (dict(ksize=1), b"ksize"),
        (dict(stride=2), b"stride"), (dict(ksize=4, stride=1), b"stride"), (dict(stride=3), b"stride"),
        (dict(c_in=48), b"c_in"), (dict(c_in=3), b"c_in"), (dict(n_out=16), b"n_out"), (dict(n_out=256), b"n_out"),
        (dict(x_dtype=_lib.PF_BF16), b"x_dtype"), (dict(x_dtype=_lib.PF_F64), b"x_dtype"),
        (dict(out_dtype=_lib.PF_BF16), b"out_dtype"), (dict(out_dtype=_lib.PF_U8), b"out_dtype"),
        (dict(x_dtype=_lib.PF_U8, c_in=3, ksize=5), b"image layer"), (dict(x_dtype=_lib.PF_F32, c_in=32), b"image layer"),
        (dict(w=3), b"w = 3"), (dict(ksize=7, c_in=64, w=2), b"pad = 3"),
        (dict(ksize=4, stride=2, h=15), b"even h and w"), (dict(ksize=4, stride=2, w=31), b"even h and w"),
        (dict(n_img=64, h=1024, w=1024), b"n_img * h * w * c_in"),
        (dict(n_img=32, h=1024, w=1024, n_out=128), b"n_img * h_out * w_out * n_out"),
        (dict(n_img=0), b"n_img"),
    ]
    for kw, needle in bad:
        assert lib.pf_pano_conv(C.byref(_desc(**kw)), None) == 1, kw
        msg = lib.pf_last_error_string()
        assert msg.startswith(b"pf_pano_conv") and needle in msg, (kw, msg)
    assert lib.pf_pano_conv(None, None) == 1
    assert lib.pf_faed_features(None, 1, 1, 1, 128, 0x10000, 0x20000, None) == 1 and b"pf_faed_features" in lib.pf_last_error_string()
    assert lib.pf_faed_features(0x10000, 1, 0, 1, 128, 0x20000, 0x30000, None) == 1


def test_tile_rows_follow_the_512_tile_threshold(monkeypatch):
    """pf_pano_conv_tile_rows: 16-row tiles at stride 1 with the 5-, 7- and 9-wide kernels from 512 tiles of 16 x 16 on (counted with
    partial tiles), 8 rows one tile short of that, always at 3 x 3 and at stride 2; PF_PANO_CONV_ROWS forces a form only where both
    exist; 0 for a geometry the launch rejects."""
    from panfusion_amd import ops
    monkeypatch.delenv("PF_PANO_CONV_ROWS", raising=False)
    for k in (5, 7, 9):
        assert ops.pano_conv_tile_rows(k, 1, 2, 256, 256) == 16            # 2 * 16 * 16 = 512 tiles
        assert ops.pano_conv_tile_rows(k, 1, 2, 256, 240) == 8             # 2 * 16 * 15 = 480
        assert ops.pano_conv_tile_rows(k, 1, 1, 511, 256) == 16            # 32 * 16: the last row of tiles is partial
        assert ops.pano_conv_tile_rows(k, 1, 1, 496, 257) == 16            # 31 * 17 = 527
        assert ops.pano_conv_tile_rows(k, 1, 1, 496, 256) == 8             # 31 * 16 = 496
        assert ops.pano_conv_tile_rows(k, 1, 4, 512, 1024) == 16           # the encoder's batch at the size in use
    assert ops.pano_conv_tile_rows(3, 1, 4, 512, 1024) == 8
    assert ops.pano_conv_tile_rows(4, 2, 4, 512, 1024) == 8
    monkeypatch.setenv("PF_PANO_CONV_ROWS", "4")
    assert ops.pano_conv_tile_rows(9, 1, 2, 19, 36) == 16
    assert ops.pano_conv_tile_rows(3, 1, 2, 19, 36) == 8 and ops.pano_conv_tile_rows(4, 2, 2, 20, 36) == 8
    monkeypatch.setenv("PF_PANO_CONV_ROWS", "2")
    assert ops.pano_conv_tile_rows(9, 1, 2, 256, 256) == 8
    lib = _lib.lib()
    for bad in ((6, 1, 1, 8, 8), (9, 2, 1, 8, 8), (4, 1, 1, 8, 8), (9, 1, 0, 8, 8), (9, 1, 1, 8, 3), (4, 2, 1, 7, 8)):
        assert lib.pf_pano_conv_tile_rows(*bad) == 0, bad
    with pytest.raises(ValueError, match="pano_conv_tile_rows"):
        ops.pano_conv_tile_rows(6, 1, 1, 8, 8)


def test_encoder_takes_three_channels_only():
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(1).items()}
    enc = M.Encoder.from_state_dict(sd, device="cpu")
    for shape in ((1, 4, 32, 64), (1, 1, 32, 64), (3, 32, 64)):
        with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
            enc(torch.zeros(shape, dtype=torch.uint8))


def test_activations_are_kept_across_a_short_last_chunk():
    """One allocation per image size serves every chunk up to the largest seen: a batch of 5 at max_batch 4 allocates once."""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(1).items()}
    enc = M.Encoder.from_state_dict(sd, device="cpu", max_batch=4)
    four = enc._activations(4, 64, 128)
    one = enc._activations(1, 64, 128)
    again = enc._activations(4, 64, 128)
    assert len(four) == 17 and four[0].shape == (4, 64, 128, 32) and four[-1].shape == (4, 2, 4, 128) and four[-1].dtype == torch.float32
    assert all(a.shape[0] == 1 and a.is_contiguous() and a.data_ptr() == b.data_ptr() for a, b in zip(one, four))
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(again, four))
    other = enc._activations(2, 32, 64)                                   # another image size replaces it: scratch stays bounded
    assert list(enc._acts) == [(32, 64)] and other[0].shape == (2, 32, 64, 32)


def test_checkpoint_is_read_with_the_tensor_only_unpickler(tmp_path):
    sd = {"net.encoder." + k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(1).items()}
    path = tmp_path / "faed.ckpt"
    torch.save({"state_dict": sd, "epoch": 3}, path)
    m = FrechetAutoEncoderDistance.from_checkpoint(str(path), pano_height=64, device="cpu")
    assert m.num_features == 256 and len(m.encoder.layers) == 17
    torch.save({"state_dict": sd, "hyper_parameters": M.Encoder}, path)  # a pickled class: refused unless trusted
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|allowlist"):
        FrechetAutoEncoderDistance.from_checkpoint(str(path), pano_height=64, device="cpu")
    assert len(FrechetAutoEncoderDistance.from_checkpoint(str(path), pano_height=64, device="cpu", trusted=True).encoder.layers) == 17
