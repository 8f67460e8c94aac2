"""Golden trajectory of known-region sampling (inpainting / outpainting) at cfg 1 (tests/test_gpu_inpaint.py).

Runs in the build container (CPU, about 20 s per step on 8 cores):

    python tools/make_golden_inpaint.py

  -> tests/golden/cfg1_inpaint_ddim10.npz   configs[0] set-up of tools/make_golden_cfg.py:cfg1 -- m = 4 horizon views of
                                            32x32 latents, 64x128 panorama latent, SD-2-base widths, the REFERENCE's own
                                            class as the denoiser, guidance 9, 90-degree rotation per step, 10 DDIM steps --
                                            with known content: the inputs of the known region and the latents after every
                                            step, panorama in the un-rotated frame.

Known content: a seeded N(0, 1) panorama latent (seed 5) kept on the columns [112, 128) and [0, 40) -- a band across the
seam -- and generated elsewhere; the views' known latents and masks are the nearest-neighbour e2p of the panorama's, as
init_noise projects the noise.  Mask convention of diffusers: 1 = generate, 0 = keep.

The blend is written out in diffusers' own form (StableDiffusionInpaintPipeline 0.24, the 4-channel branch, strength 1):
after the DDIM update of step i,

    init_latents_proper = scheduler.add_noise(z, noise, timesteps[i + 1])     (z itself at the last step)
    latents = (1 - mask) * init_latents_proper + mask * latents

in fp32, with ``noise`` the loop's starting latents.  The panorama's known latent, mask and noise are rolled with
torch.roll together with the latent before every denoiser call (PanFusion.py:149), so they stay in the latent's frame:
the naive form the kernel's offset addressing is pinned against.  The views never roll.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ddim as oddim  # noqa: E402
from oracle import fixtures as FX  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KEEP_COLUMNS = (112, 40)          # kept: [112, W) and [0, 40) of the 128-wide panorama latent


def known_inputs(cams, lat_hw, pano_hw, seed=5):
    """(view known latents (1,m,4,h,w), view masks (1,m,1,h,w), panorama known latent (1,1,4,H,W), panorama mask (1,1,1,H,W))."""
    z = torch.randn(1, 1, 4, *pano_hw, generator=torch.Generator().manual_seed(seed))
    mask = torch.ones(1, 1, 1, *pano_hw)
    mask[..., KEEP_COLUMNS[0]:] = 0.0
    mask[..., :KEEP_COLUMNS[1]] = 0.0
    _, z_views = oddim.init_noise(z, cams, *lat_hw)
    _, m_views = oddim.init_noise(mask, cams, *lat_hw)
    return z_views, m_views, z, mask


def add_noise(ddim, z, noise, t):
    """diffusers DDIMScheduler.add_noise at one timestep, fp32."""
    a = ddim.alphas_cumprod[t]
    return a ** 0.5 * z + (1 - a) ** 0.5 * noise


def rotate(x, degree):
    return torch.roll(x, int(degree / 360 * x.shape[-1]), dims=-1) if degree % 360 else x


def cfg1_inpaint_ddim10(steps=10, rot_diff=90.0, guidance_scale=9.0):
    model = FX.build_full_width()
    if os.environ.get("PF_GOLDEN_PORT", "0") != "1":
        model = FX.reference_denoiser(model)
        print("cfg1 inpaint: denoiser =", type(model).__module__, type(model).__name__, flush=True)
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    z_v, m_v, z_p, m_p = known_inputs(cams, (32, 32), (64, 128))
    n_v, n_p = latents.clone(), pano_latent.clone()          # strength 1: the noise is the starting latents
    m = latents.shape[1]
    ddim = oddim.DDIM()
    timesteps = [int(t) for t in ddim.set_timesteps(steps)]
    traj_v, traj_p = [], []
    total = 0.0
    t0 = time.time()
    with torch.no_grad(), FX.chunked_attention():
        for i, t in enumerate(timesteps):
            # PanFusion.py:149: roll the panorama -- and, here, its known latent, mask and noise -- before the call
            pano_latent, cams = oddim.rotate_latent(pano_latent, cams, rot_diff)
            z_p, m_p, n_p = rotate(z_p, rot_diff), rotate(m_p, rot_diff), rotate(n_p, rot_diff)
            total += rot_diff
            timestep = torch.full((1, m), t, dtype=torch.long)
            eps, pano_eps = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano_latent), oddim.cfg_pair(timestep),
                                  pe, ppe, oddim.cfg_pair(cams))
            eps, pano_eps = oddim.cfg_merge(eps, guidance_scale), oddim.cfg_merge(pano_eps, guidance_scale)
            latents, pano_latent = ddim.step(eps, t, latents), ddim.step(pano_eps, t, pano_latent)
            # StableDiffusionInpaintPipeline, num_channels_unet == 4
            last = i == len(timesteps) - 1
            proper_v = z_v if last else add_noise(ddim, z_v, n_v, timesteps[i + 1])
            proper_p = z_p if last else add_noise(ddim, z_p, n_p, timesteps[i + 1])
            latents = (1 - m_v) * proper_v + m_v * latents
            pano_latent = (1 - m_p) * proper_p + m_p * pano_latent
            traj_v.append(latents.numpy().copy())
            traj_p.append(rotate(pano_latent, -total).numpy().copy())           # un-rotated frame
            print("cfg1 inpaint step %d t=%d  %.0f s" % (i + 1, t, time.time() - t0), flush=True)
    z_v, m_v, z_p, m_p = known_inputs(FX.horizon4_cameras(), (32, 32), (64, 128))
    FX.save_golden(os.path.join(OUT, "cfg1_inpaint_ddim10.npz"), latents=np.stack(traj_v), pano_latent=np.stack(traj_p),
                   timesteps=np.array(timesteps, dtype=np.int64), known_latents=z_v.numpy(), known_mask=m_v.numpy(),
                   known_pano=z_p.numpy(), known_pano_mask=m_p.numpy())


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("PF_THREADS", os.cpu_count() or 8)))
    cfg1_inpaint_ddim10()
    print("done", flush=True)
