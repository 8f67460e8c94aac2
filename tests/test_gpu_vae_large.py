"""The VAE's mid-block attention in its two forms (vae.attention_plan): "flash" (pf_attention_wide) and "materialised", whole and with
its query rows cut into chunks, inside the decoder and the encoder, against the fp32 oracle at the tolerances of test_gpu_vae.py;
the host-side split of the resnets' 1x1 shortcut over pixel-row ranges (max_operand_bytes), forced at a moderate size, bit for bit.
Needs an MI355X: `-m gpu`."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _models(cfg, seed):
    from oracle import sd2_unet as U
    from oracle import vae as OV
    from panfusion_amd.models.vae_params import VAEDecoderParams, VAEEncoderParams
    ov = OV.AutoencoderKLDecoder(**cfg)
    U.init_synthetic(ov, seed)
    sd = ov.state_dict()
    dec, enc = VAEDecoderParams(**cfg), VAEEncoderParams(**cfg)
    dec.load_state_dict({k: v for k, v in sd.items() if k.startswith(("decoder.", "post_quant_conv."))}, strict=True)
    enc.load_state_dict({k: v for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))}, strict=True)
    return ov, dec, enc


@functools.lru_cache(maxsize=None)
def sd2_decode_case():
    """SD-2 widths, one 32 x 80 latent (2560 tokens at the mid-block): models, latent and the oracle's image, computed once."""
    from oracle import vae as OV
    ov, dec, enc = _models(dict(OV.SD2_VAE), 63)
    lat = torch.randn(1, 1, 4, 32, 80, generator=torch.Generator().manual_seed(17))
    with torch.no_grad():
        want = OV.decode_latent(lat, ov)
    return dec, lat, want


@functools.lru_cache(maxsize=None)
def sd2_encode_case():
    from oracle import vae as OV
    ov, dec, enc = _models(dict(OV.SD2_VAE), 64)
    x = torch.rand(1, 3, 256, 640, generator=torch.Generator().manual_seed(18)) * 2 - 1
    with torch.no_grad():
        dist = ov.encode(x).latent_dist
    return enc, x, dist.mean, dist.logvar


CHUNK_BYTES = 8 << 20                  # attention_operand_bytes lowered to this: 2560 tokens run as 4 chunks of 640 query rows


def test_decoder_sd2_widths_flash_and_chunked():
    from panfusion_amd import vae as PV
    dec, lat, want = sd2_decode_case()
    assert PV.attention_plan(1, 2560, 512, torch.float16, "materialised", CHUNK_BYTES).rows == 640
    base = PV.decode_latent(lat.to(DEV), PV.VAEDecoder(dec, compute_dtype=torch.float16))
    for name in ("flash", "chunked"):
        kw = dict(attention="flash") if name == "flash" else dict(attention="materialised", attention_operand_bytes=CHUNK_BYTES)
        d = PV.VAEDecoder(dec, compute_dtype=torch.float16, **kw)
        got = PV.decode_latent(lat.to(DEV), d)
        err = rel_l2(got.cpu(), want)
        print("VAE decode SD-2 widths 32x80, attention %s: rel-L2 vs oracle %.3e, vs the default form %.3e" % (name, err, rel_l2(got, base)))
        assert got.shape == (1, 1, 3, 256, 640) and torch.isfinite(got).all() and err <= 1e-3
    # "materialised" without a lowered limit is the default path, bit for bit
    again = PV.decode_latent(lat.to(DEV), PV.VAEDecoder(dec, compute_dtype=torch.float16, attention="materialised"))
    assert torch.equal(again, base) and rel_l2(base.cpu(), want) <= 1e-3


def test_decoder_sd2_widths_forced_splits():
    """max_operand_bytes = 50 MB: the 1x1 shortcut of up_blocks[2].resnets[0] (40 960 pixel rows x 512 fp32 channels, 84 MB) runs as 2
    row ranges, that of up_blocks[3].resnets[0] (163 840 x 256, 168 MB) as 4; the 3x3 up-sampling convolution of up_blocks[1]
    (fp32 output 128 x 320 x 512, 84 MB) runs in 2 row bands with a one-row halo, that of up_blocks[2] (256 x 640 x 256, 168 MB) in 4.
    Bit-identical to the unsplit decode, with the materialised attention and with the flash kernel."""
    from panfusion_amd import engine
    from panfusion_amd import vae as PV
    dec, lat, want = sd2_decode_case()
    limit = 50 << 20
    assert len(engine.row_ranges(40960, 2048, limit)) == 2 and len(engine.row_ranges(163840, 1024, limit)) == 4
    row1, row2 = 2 * 320 * 512 * 4, 2 * 640 * 256 * 4                       # bytes of the two output rows of one input row
    assert len(engine.row_ranges(64, row1, limit - 2 * row1)) == 2 and len(engine.row_ranges(128, row2, limit - 2 * row2)) == 4
    for attention in ("materialised", "flash"):
        base = PV.decode_latent(lat.to(DEV), PV.VAEDecoder(dec, compute_dtype=torch.float16, attention=attention))
        got = PV.decode_latent(lat.to(DEV), PV.VAEDecoder(dec, compute_dtype=torch.float16, attention=attention, max_operand_bytes=limit))
        assert torch.equal(got, base), "split shortcut differs from the unsplit one (%s): rel-L2 %.3e" % (attention, rel_l2(got, base))
        assert rel_l2(got.cpu(), want) <= 1e-3


def test_encoder_sd2_widths_flash_and_chunked():
    from panfusion_amd import vae as PV
    enc, x, mean, logvar = sd2_encode_case()
    base = PV.VAEEncoder(enc, compute_dtype=torch.float16).moments(x.to(DEV))
    for name in ("flash", "chunked"):
        kw = dict(attention="flash") if name == "flash" else dict(attention="materialised", attention_operand_bytes=CHUNK_BYTES)
        e = PV.VAEEncoder(enc, compute_dtype=torch.float16, **kw)
        gm, gl = e.encode(x.to(DEV))
        em, el = rel_l2(gm.cpu(), mean), rel_l2(gl.cpu(), logvar)
        print("VAE encode SD-2 widths 256x640, attention %s: mean %.3e logvar %.3e" % (name, em, el))
        assert gm.shape == (1, 4, 32, 80) and max(em, el) <= 1e-3
    again = PV.VAEEncoder(enc, compute_dtype=torch.float16, attention="materialised").moments(x.to(DEV))
    assert torch.equal(again, base)


def test_encoder_sd2_widths_forced_shortcut_split():
    """max_operand_bytes = 30 MB: the shortcut of down_blocks[1].resnets[0] (40 960 pixel rows, 128 -> 256 channels: 42 MB of fp32
    output) runs as 2 row ranges.  Moments bit-identical to the unsplit encode and within 1e-3 of the oracle."""
    from panfusion_amd import vae as PV
    enc, x, mean, logvar = sd2_encode_case()
    base = PV.VAEEncoder(enc, compute_dtype=torch.float16).moments(x.to(DEV))
    e = PV.VAEEncoder(enc, compute_dtype=torch.float16, max_operand_bytes=30 << 20)
    got = e.moments(x.to(DEV))
    assert torch.equal(got, base), "split shortcut differs from the unsplit one: rel-L2 %.3e" % rel_l2(got, base)
    gm, gl = e.encode(x.to(DEV))
    assert max(rel_l2(gm.cpu(), mean), rel_l2(gl.cpu(), logvar)) <= 1e-3


@pytest.mark.parametrize("attention", ["flash", "materialised"])
@pytest.mark.parametrize("dtype,precision,tol", [(torch.float16, "mixed", 1e-3), (torch.float16, "fast", 4e-3), (torch.bfloat16, "fast", 3e-2)])
def test_tiny_width_128_both_forms(dtype, precision, tol, attention):
    """Block widths (64, 64, 128, 128): the mid-block attention has C = 128, the narrowest head the flash kernel serves.  Decode and
    encode in both attention forms, each within the tiny tests' tolerance of the oracle."""
    from oracle import vae as OV
    from panfusion_amd import vae as PV
    cfg = dict(OV.tiny_vae_config(width=64, groups=8), block_out_channels=(64, 64, 128, 128))
    ov, dec, enc = _models(cfg, 65)
    assert ov.decoder.mid_block.attentions[0].to_q.weight.shape[0] == 128
    g = torch.Generator().manual_seed(19)
    lat = torch.randn(1, 2, 4, 16, 24, generator=g)
    with torch.no_grad():
        want = OV.decode_latent(lat, ov)
    got = PV.decode_latent(lat.to(DEV), PV.VAEDecoder(dec, compute_dtype=dtype, precision=precision, attention=attention))
    ed = rel_l2(got.cpu(), want)
    x = torch.rand(2, 3, 64, 192, generator=g) * 2 - 1
    with torch.no_grad():
        dist = ov.encode(x).latent_dist
    gm, gl = PV.VAEEncoder(enc, compute_dtype=dtype, precision=precision, attention=attention).encode(x.to(DEV))
    em, el = rel_l2(gm.cpu(), dist.mean), rel_l2(gl.cpu(), dist.logvar)
    print("VAE tiny C = 128 %s/%s attention %s: decode %.2e, encode mean %.2e logvar %.2e" % (dtype, precision, attention, ed, em, el))
    assert max(ed, em, el) <= tol


def test_flash_refuses_what_the_kernel_does_not_serve():
    """A mid-block width of 64 is not one the flash kernel serves: ValueError, no fall-back to the materialised form."""
    from oracle import vae as OV
    from panfusion_amd import vae as PV
    cfg = dict(OV.tiny_vae_config(width=64, groups=8), block_out_channels=(64, 64, 64, 64))
    ov, dec, enc = _models(cfg, 66)
    with pytest.raises(ValueError, match="flash"):
        PV.decode_latent(torch.randn(1, 1, 4, 8, 8).to(DEV), PV.VAEDecoder(dec, compute_dtype=torch.float16, attention="flash"))


# ------------------------------------------------------------------------------------------------ 1024 x 2048 (padded: 1024 x 2176)
def _sd2_synthetic(cls, seed):
    from panfusion_amd.models.sd2_unet_params import fill_synthetic
    from panfusion_amd.models.vae_params import SD2_VAE
    with torch.device(DEV):
        params = cls(**SD2_VAE)
    fill_synthetic(params, seed)
    return params


def test_full_size_decode_views_and_pano():
    """decode_views_and_pano of a seeded (1, 1, 4, 128, 256) panorama latent (latent_pad 8: 128 x 272 -> 1024 x 2176, 34 816 tokens at the
    mid-block) and one 64 x 64 view, SD-2 widths, synthetic weights, fp16 mixed: shape and finiteness, and the fp32 panorama images of
    the two attention forms (flash; query-chunked materialised) within 2e-3 rel-L2 -- the triangle bound of two paths each gated at
    1e-3 against the oracle.  On the way: the 1x1 shortcut of up_blocks[3].resnets[0] in 2 pixel-row ranges and the up-sampling
    convolution of up_blocks[2] (2.28 GB of fp32 output) in row bands."""
    from panfusion_amd import vae as PV
    from panfusion_amd.models.vae_params import VAEDecoderParams
    from panfusion_amd.utils.pano import pad_pano
    params = _sd2_synthetic(VAEDecoderParams, 9)
    g = torch.Generator().manual_seed(21)
    lat, pano = torch.randn(1, 1, 4, 64, 64, generator=g).to(DEV), torch.randn(1, 1, 4, 128, 256, generator=g).to(DEV)
    dec = PV.VAEDecoder(params, compute_dtype=torch.float16, attention="flash")
    images, pano_img = PV.decode_views_and_pano(lat, pano, dec, latent_pad=8)
    assert images.shape == (1, 1, 512, 512, 3) and pano_img.shape == (1, 1, 1024, 2048, 3) and pano_img.dtype == torch.uint8
    a = PV.decode_latent(pad_pano(pano, 8), dec)
    assert a.shape == (1, 1, 3, 1024, 2176) and torch.isfinite(a).all()
    b = PV.decode_latent(pad_pano(pano, 8), PV.VAEDecoder(params, compute_dtype=torch.float16, attention="materialised"))
    err = rel_l2(a, b)
    print("VAE decode 1024 x 2176, fp16 mixed: flash vs query-chunked materialised rel-L2 %.3e (bound 2e-3)" % err)
    assert torch.isfinite(b).all() and err <= 2e-3


def test_full_size_encode():
    """VAEEncoder.encode of a seeded (1, 3, 1024, 2176) image, SD-2 widths, synthetic weights: shape, finiteness and the two attention
    forms' agreement on the mean (2e-3 rel-L2)."""
    from panfusion_amd import vae as PV
    from panfusion_amd.models.vae_params import VAEEncoderParams
    params = _sd2_synthetic(VAEEncoderParams, 10)
    x = (torch.rand(1, 3, 1024, 2176, generator=torch.Generator().manual_seed(22)) * 2 - 1).to(DEV)
    ma, la = PV.VAEEncoder(params, compute_dtype=torch.float16, attention="flash").encode(x)
    mb, lb = PV.VAEEncoder(params, compute_dtype=torch.float16, attention="materialised").encode(x)
    assert ma.shape == la.shape == (1, 4, 128, 272) and all(torch.isfinite(t).all() for t in (ma, la, mb, lb))
    err = rel_l2(ma, mb)
    print("VAE encode 1024 x 2176, fp16 mixed: mean, flash vs query-chunked materialised rel-L2 %.3e (bound 2e-3)" % err)
    assert err <= 2e-3


def test_source_latents_from_a_1024x2048_panorama():
    """SourceLatents.from_panorama on a 1024 x 2048 panorama with 2 cameras returns latents of the cfg 4 shapes."""
    from panfusion_amd import vae as PV
    from panfusion_amd.models.vae_params import VAEEncoderParams
    from panfusion_amd.pipeline import SourceLatents
    enc = PV.VAEEncoder(_sd2_synthetic(VAEEncoderParams, 10), compute_dtype=torch.float16)
    pano = (torch.rand(1, 1, 3, 1024, 2048, generator=torch.Generator().manual_seed(23)) * 2 - 1).to(DEV)
    cams = {"FoV": torch.full((1, 2), 90), "theta": torch.tensor([[0., 180.]], dtype=torch.float64), "phi": torch.tensor([[0., 10.]], dtype=torch.float64)}
    src = SourceLatents.from_panorama(enc, pano, cams, (64, 64))
    assert src.latents.shape == (1, 2, 4, 64, 64) and src.pano_latent.shape == (1, 1, 4, 128, 256)
    assert torch.isfinite(src.latents).all() and torch.isfinite(src.pano_latent).all()
