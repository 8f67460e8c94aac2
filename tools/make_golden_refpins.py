"""tests/golden/ref_pins.npz and tests/golden/ref_cfg1_call.npz from the REFERENCE'S OWN code: the recorded answers that
tests/test_oracle_vs_reference.py pins oracle/*.py against, so that those tests run on every machine without the reference
tree.  Same inputs as the tests (all seeded), same comparisons: what the tests check bit-exactly is stored as a SHA-256 digest
of the value (dtype-agnostic, -0.0 == +0.0: the semantics of np.array_equal / torch.equal), what they check to a tolerance is
stored as the array itself.  Before it writes anything the script runs the oracle on the same inputs and checks that every
pin holds.

Runs only where the reference tree is importable (oracle/ref_import.py; scipy for py360convert):

    python tools/make_golden_refpins.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import fixtures as FX  # noqa: E402
from oracle import geometry as G  # noqa: E402
from oracle import mvgen as MV  # noqa: E402
from oracle import py360  # noqa: E402
from oracle import ref_import  # noqa: E402
from oracle import sd2_unet as U  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GRID_SIZES = ((64, 128, 64, 64), (32, 64, 32, 32), (16, 32, 16, 16), (8, 16, 8, 8), (128, 256, 64, 64))
PE_FREQS = (16, 80, 160, 320)
PE_SAMPLE = 16384


def digest(*arrays):
    """SHA-256 of the VALUES of a sequence of arrays (copy of tests/test_oracle_vs_reference.py:digest)."""
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.dtype.kind == "f":
            a = a.astype(np.float64) + 0.0
        elif a.dtype.kind in "iu":
            a = a.astype(np.int64)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def cam4():
    return {"FoV": torch.full((4,), 90), "theta": torch.tensor([0., 90, 180, 270], dtype=torch.float64),
            "phi": torch.tensor([0., 10, -20, 45], dtype=torch.float64)}


def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def remap_inputs():
    g = torch.Generator().manual_seed(31)
    return torch.randn(20, 3, 16, 32, generator=g), torch.randn(20, 3, 16, 16, generator=g)


def pad_inputs():
    g = torch.Generator().manual_seed(32)
    return torch.randn(2, 3, 5, 16, generator=g), torch.randn(2, 2, 3, 5, 16, generator=g)


def warpattn_inputs():
    g = torch.Generator().manual_seed(33)
    return torch.randn(4, 64, 8, 8, generator=g), torch.randn(1, 64, 8, 16, generator=g)


def tiny_denoiser_setup():
    cfg = U.tiny_config(width=32, cross_attention_dim=64, heads=(1, 2, 4, 4), groups=8)
    unet, pano_unet = U.UNet2DConditionModel(**cfg), U.UNet2DConditionModel(**cfg)
    unet.add_lora(4)
    U.init_synthetic(unet, 1)
    U.init_synthetic(pano_unet, 2)
    g = torch.Generator().manual_seed(34)
    b, m = 2, 4
    args = (torch.randn(b, m, 4, 16, 16, generator=g), torch.randn(b, 1, 4, 16, 32, generator=g), torch.full((b, m), 981),
            torch.randn(b, m, 7, 64, generator=g), torch.randn(b, 1, 7, 64, generator=g),
            {k: torch.stack([v, v]) for k, v in cam4().items()})
    return unet, pano_unet, args


def py360_cases():
    """The 12 random trials of test_py360_e2p_bit_exact: (img, fov, u, v, hw, rot)."""
    rng = np.random.default_rng(11)
    cases = []
    for trial in range(12):
        H = int(rng.integers(9, 40))
        W = 2 * H + int(rng.integers(0, 3))
        img = (rng.random((H, W, 3)) * 255).astype(np.uint8) if trial % 3 == 0 else \
            rng.standard_normal((H, W, 2)).astype(np.float32) if trial % 3 == 1 else rng.standard_normal((H, W)).astype(np.float32)
        u, v = float(rng.uniform(-180, 180)), float(rng.uniform(-90, 90))
        fov = (float(rng.uniform(40, 120)), float(rng.uniform(40, 120)))
        hw = (int(rng.integers(5, 30)), int(rng.integers(5, 30)))
        rot = float(rng.uniform(-30, 30)) if trial % 4 == 0 else 0
        cases.append((img, fov, u, v, hw, rot))
    return cases


def main():
    ref = ref_import.load()
    out = {}

    # cameras: the reference's samplers, values as they are
    np.random.seed(123)
    out["random_theta"], out["random_phi"] = (np.asarray(x) for x in ref.random_sample_camera(20))
    out["ico_theta"], out["ico_phi"] = (np.asarray(x) for x in ref.icosahedron_sample_camera())
    out["horizon8_theta"], out["horizon8_phi"] = (np.asarray(x) for x in ref.horizon_sample_camera(8))
    thd, phd = np.degrees(out["ico_theta"]), np.degrees(out["ico_phi"])

    # e2p / p2e grids: one digest per (rotation, size, direction) over all 20 cameras
    for rot in (0, 90, 180, 270):
        e2p, p2e = [], []
        for eh, ew, h, w in GRID_SIZES:
            t = [(thd[i] + rot) % 360 for i in range(20)]
            e2p.append(digest(*[a for i in range(20) for a in ref.map_pers_pix_to_equi(eh, ew, 90, t[i], phd[i], h, w)]))
            p2e.append(digest(*[a for i in range(20) for a in ref.map_equi_pix_to_pers(h, w, 90, t[i], phd[i], eh, ew)]))
            assert np.array_equal(e2p[-1], digest(*[a for i in range(20) for a in G.e2p_grid(eh, ew, 90, t[i], phd[i], h, w)]))
            assert np.array_equal(p2e[-1], digest(*[a for i in range(20) for a in G.p2e_grid(h, w, 90, t[i], phd[i], eh, ew)]))
        out["grid_e2p_rot%d" % rot], out["grid_p2e_rot%d" % rot] = np.stack(e2p), np.stack(p2e)

    # remap modes
    x, y = remap_inputs()
    cams = (torch.full((20,), 90), torch.tensor(thd), torch.tensor(phd))
    for mode in ("nearest", "bilinear", None):
        out["e2p_%s" % mode] = digest(ref.e2p(x, *cams, (16, 16), mode=mode))
        assert np.array_equal(out["e2p_%s" % mode], digest(G.e2p(x, *cams, (16, 16), mode=mode)))
    out["p2e"] = digest(*ref.p2e(y, *cams, (16, 32)))
    out["e2p_scalar_camera"] = digest(ref.e2p(x, 90, 30.0, 10.0, (8, 8)))
    assert np.array_equal(out["p2e"], digest(*G.p2e(y, *cams, (16, 32))))
    assert np.array_equal(out["e2p_scalar_camera"], digest(G.e2p(x, 90, 30.0, 10.0, (8, 8))))

    # EPA masks, coordinates, spherical PE
    camd = {"FoV": torch.full((20,), 90), "theta": torch.tensor((thd + 180) % 360), "phi": torch.tensor(phd)}
    out["masks"] = digest(*ref.get_masks(8, 8, 8, 16, camd, "cpu"))
    coords = ref.get_coords(16, 16, 16, 32, camd, "cpu")
    out["coords"] = digest(*coords)
    assert np.array_equal(out["masks"], digest(*G.get_masks(8, 8, 8, 16, camd)))
    assert np.array_equal(out["coords"], digest(*G.get_coords(16, 16, 16, 32, camd)))
    for n in PE_FREQS:
        pe = ref.SphericalPE(n)
        # sin / cos of float32 arguments up to 2^63 round differently by one unit in the last place on different host CPUs:
        # the PE is stored as values (a seeded sample of PE_SAMPLE entries) and compared to within one ulp
        val = pe(coords[0]).reshape(-1)
        idx = np.sort(np.random.default_rng(n).choice(val.numel(), PE_SAMPLE, replace=False))
        out["pe%d_freq" % n], out["pe%d_idx" % n], out["pe%d_val" % n] = digest(pe.freq_bands), idx, val[idx].numpy()
        assert np.array_equal(out["pe%d_freq" % n], digest(G.spherical_freq_bands(n)))
        assert np.array_equal(G.spherical_pe(G.get_coords(16, 16, 16, 32, camd)[0], pe.freq_bands).reshape(-1)[idx].numpy(), val[idx].numpy())

    # panorama padding
    xs = pad_inputs()
    out["pad2"] = np.stack([digest(ref.pad_pano(a, 2)) for a in xs])
    out["unpad_roundtrip"] = np.array([torch.equal(ref.unpad_pano(ref.pad_pano(a, 3), 3), a) for a in xs])
    assert all(np.array_equal(d, digest(G.pad_pano(a, 2))) for d, a in zip(out["pad2"], xs))

    # WarpAttn: identity at construction, then seeded weights
    torch.manual_seed(0)
    wa = ref.WarpAttn(64)
    px, ex = warpattn_inputs()
    with torch.no_grad():
        po, eo = wa(px, ex, cam4())
    out["warpattn_identity_at_init"] = np.array(torch.equal(po, px) and torch.equal(eo, ex))
    U.init_synthetic(wa, 3)
    MV.randomize_epa(wa, 4)
    sd = wa.state_dict()
    out["warpattn_keys"] = np.array(["%s %s" % (k, tuple(v.shape)) for k, v in sd.items()])
    out["warpattn_weights"] = digest(*sd.values())
    with torch.no_grad():
        a = wa(px, ex, cam4())
    out["warpattn_pers_out"], out["warpattn_equi_out"] = a[0].numpy(), a[1].numpy()
    blk = MV.EPABlock(64)
    U.init_synthetic(blk, 3)
    MV.randomize_epa(blk, 4)
    assert np.array_equal(out["warpattn_weights"], digest(*blk.state_dict().values()))

    # the denoiser, tiny widths
    unet, pano_unet, args = tiny_denoiser_setup()
    rm = ref.MultiViewBaseModel(unet, pano_unet, None, None, True)
    torch.manual_seed(35)                      # the EPA weights that randomize_epa leaves at their default initialisation
    om = MV.DualBranchDenoiser(unet, pano_unet, None, None, True)
    MV.randomize_epa(om, 5)
    rm.load_state_dict({k: v for k, v in om.state_dict().items() if k.startswith("cp_blocks")}, strict=False)
    with torch.no_grad():
        a, o = rm(*args), om(*args)
    out["denoiser_sample"], out["denoiser_pano_sample"] = a[0].numpy(), a[1].numpy()
    assert rel_l2(o[0], a[0]) < 1e-5 and rel_l2(o[1], a[1]) < 1e-5

    # py360convert e2p
    dig, dts = [], []
    for img, fov, u, v, hw, rot in py360_cases():
        for mode in ("bilinear", "nearest"):
            want = ref.py360_e2p(img, fov, u, v, hw, in_rot_deg=rot, mode=mode)
            got = py360.e2p(img, fov, u, v, hw, in_rot_deg=rot, mode=mode)
            assert got.dtype == want.dtype and np.array_equal(got, want)
            dig.append(digest(want))
            dts.append(want.dtype.str)
    out["py360_e2p"], out["py360_e2p_dtype"] = np.stack(dig), np.array(dts)

    p = os.path.join(OUT, "ref_pins.npz")
    np.savez_compressed(p, **out)
    print(p, os.path.getsize(p) // 1024, "KiB", flush=True)

    # the reference class at SD-2-base widths: configs[0]'s first denoiser call (minutes on the host cores)
    om = FX.build_full_width()
    rm = FX.reference_denoiser(om)
    call = FX.first_step_call(FX.horizon4_cameras(), (32, 32), (64, 128), cfg_pair=True)
    with torch.no_grad(), FX.chunked_attention():
        a = rm(call["latents"], call["pano_latent"], call["timestep"], call["prompt_embd"], call["pano_prompt_embd"], call["cameras"])
        o = om(call["latents"], call["pano_latent"], call["timestep"], call["prompt_embd"], call["pano_prompt_embd"], call["cameras"])
    ev, ep = rel_l2(o[0], a[0]), rel_l2(o[1], a[1])
    print("cfg 1 first call, port vs reference class: views %.2e  pano %.2e" % (ev, ep), flush=True)
    assert ev < 1e-5 and ep < 1e-5
    p = os.path.join(OUT, "ref_cfg1_call.npz")
    np.savez_compressed(p, sample=a[0].numpy(), pano_sample=a[1].numpy())
    print(p, os.path.getsize(p) // 1024, "KiB", flush=True)


if __name__ == "__main__":
    main()
