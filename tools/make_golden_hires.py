"""Golden trajectory of the refine pass of two-pass high-resolution sampling at cfg 1 (tests/test_gpu_hires.py).

Runs in the build container (CPU, about 20 s per step on 8 cores, six denoiser calls):

    python tools/make_golden_hires.py

  -> tests/golden/cfg1_hires_ddim10.npz     configs[0] set-up of tools/make_golden_cfg.py:cfg1 -- m = 4 horizon views of 32x32
                                            latents, 64x128 panorama latent, SD-2-base widths, the REFERENCE's own class as the
                                            denoiser, guidance 9, 90-degree rotation per step -- on the 10-step grid at strength
                                            0.6 (the 6 DDIM steps from t = 501), started from a HALF-SIZE source up-sampled 2x.

Source z: the seeded N(0, 1) panorama latent of make_golden_inpaint.known_inputs (seed 5) at 32x64 and its nearest e2p into 16x16
views.  Both are up-sampled with torch's bicubic (align_corners=False, no antialiasing):

    views      F.interpolate(z, size=(32, 32), mode="bicubic", align_corners=False)                (columns clamp)
    panorama   F.interpolate(torch.cat([z, z, z], -1), size=(64, 3 * 128), ...)[..., 128:256]      (columns periodic)

-- the panorama in the naive tripled form: the middle copy never sees the clamp at the ends.  Then make_golden_strength.py's
run, literally: add_noise start at timesteps[0], the loop over the sliced timesteps with the panorama rolled before every call.

The file holds the low-resolution source (what the test passes to SourceLatents(..., resample="bicubic")), the up-sampled
source, the executed timesteps, the start state (panorama before its first roll) and the latents after every executed step,
panorama in the un-rotated frame.
"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ddim as oddim  # noqa: E402
from oracle import fixtures as FX  # noqa: E402
from make_golden_inpaint import add_noise, known_inputs, rotate  # noqa: E402
from make_golden_strength import get_timesteps  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def upsample_clamped(z, size, mode="bicubic"):
    """(1, m, 4, h, w) -> (1, m, 4, *size): torch's own resize, every border clamped."""
    kw = {} if mode == "nearest" else dict(align_corners=False)
    return F.interpolate(z[0], size=size, mode=mode, **kw)[None]


def upsample_wrapped(z, size, mode="bicubic"):
    """The same with periodic columns, stated naively: three copies side by side, resized, the middle one cut out."""
    kw = {} if mode == "nearest" else dict(align_corners=False)
    W = size[1]
    return F.interpolate(torch.cat([z[0]] * 3, -1), size=(size[0], 3 * W), mode=mode, **kw)[None, ..., W:2 * W]


def run(name, model, steps=10, strength=0.6, rot_diff=90.0, guidance_scale=9.0, lat_hw=(32, 32), pano_hw=(64, 128)):
    cams = FX.horizon4_cameras()
    n_v, n_p, pe, ppe = FX.loop_inputs(cams, lat_hw, pano_hw)
    low_v, _, low_p, _ = known_inputs(cams, (lat_hw[0] // 2, lat_hw[1] // 2), (pano_hw[0] // 2, pano_hw[1] // 2))
    z_v, z_p = upsample_clamped(low_v, lat_hw), upsample_wrapped(low_p, pano_hw)
    m = n_v.shape[1]
    ddim = oddim.DDIM()
    timesteps, _ = get_timesteps([int(t) for t in ddim.set_timesteps(steps)], strength)
    latents, pano_latent = add_noise(ddim, z_v, n_v, timesteps[0]), add_noise(ddim, z_p, n_p, timesteps[0])
    arrays = dict(lowres_latents=low_v.numpy().copy(), lowres_pano=low_p.numpy().copy(), source_latents=z_v.numpy().copy(),
                  source_pano=z_p.numpy().copy(), start_latents=latents.numpy().copy(), start_pano=pano_latent.numpy().copy(),
                  timesteps=np.array(timesteps, dtype=np.int64))
    traj_v, traj_p = [], []
    total = 0.0
    t0 = time.time()
    with torch.no_grad(), FX.chunked_attention():
        for j, t in enumerate(timesteps):
            pano_latent, cams = oddim.rotate_latent(pano_latent, cams, rot_diff)           # PanFusion.py:149
            total += rot_diff
            timestep = torch.full((1, m), t, dtype=torch.long)
            eps, pano_eps = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano_latent), oddim.cfg_pair(timestep),
                                  pe, ppe, oddim.cfg_pair(cams))
            eps, pano_eps = oddim.cfg_merge(eps, guidance_scale), oddim.cfg_merge(pano_eps, guidance_scale)
            latents, pano_latent = ddim.step(eps, t, latents), ddim.step(pano_eps, t, pano_latent)
            traj_v.append(latents.numpy().copy())
            traj_p.append(rotate(pano_latent, -total).numpy().copy())           # un-rotated frame
            print("%s step %d t=%d  %.0f s" % (name, j + 1, t, time.time() - t0), flush=True)
    FX.save_golden(os.path.join(OUT, name + ".npz"), latents=np.stack(traj_v), pano_latent=np.stack(traj_p), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("PF_THREADS", os.cpu_count() or 8)))
    model = FX.build_full_width()
    if os.environ.get("PF_GOLDEN_PORT", "0") != "1":
        model = FX.reference_denoiser(model)
        print("cfg1 hires: denoiser =", type(model).__module__, type(model).__name__, flush=True)
    run("cfg1_hires_ddim10", model)
    print("done", flush=True)
