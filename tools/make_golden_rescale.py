"""Golden trajectory of guidance rescale at cfg 1 (tests/test_gpu_rescale.py).

Runs in the build container (CPU, about 20 s per step on 8 cores):

    python tools/make_golden_rescale.py

  -> tests/golden/cfg1_rescale_ddim10.npz   configs[0] set-up of tools/make_golden_cfg.py:cfg1 -- m = 4 horizon views of
                                            32x32 latents, 64x128 panorama latent, SD-2-base widths, the REFERENCE's own
                                            class as the denoiser, guidance 9, 90-degree rotation per step, 10 DDIM steps --
                                            with guidance_rescale = 0.7: the latents after every step (panorama in the
                                            un-rotated frame) and the two factors (views, panorama) of every step.

The rescale is diffusers' own function (StableDiffusionPipeline 0.24, pipeline_stable_diffusion.py: rescale_noise_cfg),
transcribed below and applied in fp32 to the merged predictions right before scheduler.step, on the reference's own layouts
(PanFusion.py:156-162: noise_pred (b, m, 4, h, w), pano_noise_pred (b, 1, 4, H, W)): one statistic per sample over all m
views, a separate one for the panorama.  The factor stored per latent is  phi std_text / std_cfg + 1 - phi.

Condition on the fixture, asserted here: at EVERY step at least one of the two factors lies outside [0.98, 1.02] -- else a
test could not tell the feature from its absence.  With the seeded random weights the conditional and unconditional
predictions may differ too little for that; the conditional prompt embeddings (views and panorama; not the null prompt) are
then multiplied by a constant, doubled until the condition holds.  PROMPT_SCALE below is the constant the committed fixture was
written with; it is stored in the npz (``prompt_scale``) and the GPU test applies it to the same seeded embeddings.
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
PHI = 0.7
PROMPT_SCALE = 1.0                # first constant tried; see the docstring
BAND = (0.98, 1.02)


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers 0.24 pipeline_stable_diffusion.py: rescale_noise_cfg, literally; the factor returned too."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    noise_cfg = guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg
    return noise_cfg, float(guidance_rescale * (std_text / std_cfg) + (1 - guidance_rescale))


def rotate(x, degree):
    return torch.roll(x, int(degree / 360 * x.shape[-1]), dims=-1) if degree % 360 else x


def trajectory(model, prompt_scale, steps, rot_diff, guidance_scale):
    """The loop of PanFusion.py:146-164 with the rescale; None as soon as a step has both factors inside BAND."""
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    pe, ppe = torch.cat([pe[:1], pe[1:] * prompt_scale]), torch.cat([ppe[:1], ppe[1:] * prompt_scale])
    m = latents.shape[1]
    ddim = oddim.DDIM()
    timesteps = [int(t) for t in ddim.set_timesteps(steps)]
    traj_v, traj_p, factors = [], [], []
    total = 0.0
    t0 = time.time()
    with torch.no_grad(), FX.chunked_attention():
        for i, t in enumerate(timesteps):
            pano_latent, cams = oddim.rotate_latent(pano_latent, cams, rot_diff)
            total += rot_diff
            timestep = torch.full((1, m), t, dtype=torch.long)
            eps, pano_eps = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano_latent), oddim.cfg_pair(timestep),
                                  pe, ppe, oddim.cfg_pair(cams))
            eps, f_v = rescale_noise_cfg(oddim.cfg_merge(eps, guidance_scale), eps.chunk(2)[1], PHI)
            pano_eps, f_p = rescale_noise_cfg(oddim.cfg_merge(pano_eps, guidance_scale), pano_eps.chunk(2)[1], PHI)
            print("cfg1 rescale (prompt x %g) step %d t=%d  factors %.4f / %.4f  %.0f s"
                  % (prompt_scale, i + 1, t, f_v, f_p, time.time() - t0), flush=True)
            if all(BAND[0] <= f <= BAND[1] for f in (f_v, f_p)):
                return None
            latents, pano_latent = ddim.step(eps, t, latents), ddim.step(pano_eps, t, pano_latent)
            traj_v.append(latents.numpy().copy())
            traj_p.append(rotate(pano_latent, -total).numpy().copy())           # un-rotated frame
            factors.append((f_v, f_p))
    return dict(latents=np.stack(traj_v), pano_latent=np.stack(traj_p), factors=np.array(factors, dtype=np.float32),
                timesteps=np.array(timesteps, dtype=np.int64))


def cfg1_rescale_ddim10(steps=10, rot_diff=90.0, guidance_scale=9.0):
    model = FX.build_full_width()
    if os.environ.get("PF_GOLDEN_PORT", "0") != "1":
        model = FX.reference_denoiser(model)
        print("cfg1 rescale: denoiser =", type(model).__module__, type(model).__name__, flush=True)
    scale = PROMPT_SCALE
    while True:
        out = trajectory(model, scale, steps, rot_diff, guidance_scale)
        if out is not None:
            break
        print("cfg1 rescale: both factors inside [%g, %g] at that step with the prompt x %g: doubling it" % (*BAND, scale), flush=True)
        scale *= 2.0
        assert scale <= 1024.0, "no prompt scale up to 1024 separates the rescaled run from the plain one"
    assert all(not (BAND[0] <= f[0] <= BAND[1]) or not (BAND[0] <= f[1] <= BAND[1]) for f in out["factors"])
    assert all(np.isfinite(v).all() for v in out.values())
    FX.save_golden(os.path.join(OUT, "cfg1_rescale_ddim10.npz"), prompt_scale=np.float32(scale), phi=np.float32(PHI), **out)
    print("cfg1 rescale: written with prompt_scale = %g (PROMPT_SCALE in this file should say so)" % scale, flush=True)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("PF_THREADS", os.cpu_count() or 8)))
    cfg1_rescale_ddim10()
    print("done", flush=True)
