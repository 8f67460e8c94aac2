"""Golden trajectories of strength < 1 sampling from a source panorama at cfg 1 (tests/test_gpu_strength.py).

Runs in the build container (CPU, about 20 s per step on 8 cores, twelve denoiser calls):

    python tools/make_golden_strength.py

  -> tests/golden/cfg1_strength06_ddim10.npz            configs[0] set-up of tools/make_golden_cfg.py:cfg1 -- m = 4 horizon
                                                        views of 32x32 latents, 64x128 panorama latent, SD-2-base widths, the
                                                        REFERENCE's own class as the denoiser, guidance 9, 90-degree rotation
                                                        per step -- on the 10-step grid at strength 0.6: the 6 DDIM steps from
                                                        t = 501, no mask.
  -> tests/golden/cfg1_strength06_inpaint_dpmpp10.npz   the same run with the seam-crossing kept band of
                                                        tools/make_golden_inpaint.py and the DPM-Solver++(2M) update: first
                                                        order at the first executed step and (n = 10 < 15) at the last.

Each holds the source z (views and panorama), the executed timesteps, the start state (panorama before its first roll) and the
latents after every executed step, panorama in the un-rotated frame; the second one the masks too.

Source z: the seeded N(0, 1) panorama latent of make_golden_inpaint.known_inputs (seed 5) and its nearest e2p into the views.
The noise n is the loop's usual starting noise (oracle.fixtures.loop_inputs).

Written in diffusers' own form (StableDiffusionImg2ImgPipeline / StableDiffusionInpaintPipeline 0.24):

    t_start = n - min(int(n * strength), n);  timesteps = scheduler.timesteps[t_start:]
    latents = scheduler.add_noise(z, noise, timesteps[:1])                 (everywhere, also where the mask says "generate")

then the loop of tools/make_golden_inpaint.py over the sliced timesteps (fp32; the panorama's z, mask, noise and x0 history
rolled with torch.roll together with the latent before every call -- the naive form), with the update of
tools/make_golden_dpmpp.py for 2M: the scheduler keeps the full grid, so ``lower_order_final`` looks at n = 10 and the s1 of a
second-order step is the previous executed timestep; the first executed step has no history and is first order
(``lower_order_nums < 1``).
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ddim as oddim  # noqa: E402
from oracle import fixtures as FX  # noqa: E402
from make_golden_dpmpp import DPMSolverPP2M  # noqa: E402
from make_golden_inpaint import add_noise, known_inputs, rotate  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def get_timesteps(timesteps, strength):
    """diffusers' pipelines: (timesteps[t_start:], t_start)."""
    n = len(timesteps)
    init_timestep = min(int(n * strength), n)
    t_start = max(n - init_timestep, 0)
    return timesteps[t_start:], t_start


class StartedPP2M(DPMSolverPP2M):
    """DPMSolverPP2M whose first executed step is grid index i0 (no history there: first order)."""

    def __init__(self, n, i0):
        super().__init__(n)
        self.i0 = i0

    def order(self, i):
        return 1 if i == self.i0 else super().order(i)


def run(name, model, sampler, masked, steps=10, strength=0.6, rot_diff=90.0, guidance_scale=9.0):
    cams = FX.horizon4_cameras()
    n_v, n_p, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    z_v, m_v, z_p, m_p = known_inputs(cams, (32, 32), (64, 128))
    if not masked:
        m_v, m_p = torch.ones_like(m_v), torch.ones_like(m_p)
    m = n_v.shape[1]
    ddim = oddim.DDIM()
    timesteps, i0 = get_timesteps([int(t) for t in ddim.set_timesteps(steps)], strength)
    solver = StartedPP2M(steps, i0) if sampler == "dpmpp_2m" else None
    latents, pano_latent = add_noise(ddim, z_v, n_v, timesteps[0]), add_noise(ddim, z_p, n_p, timesteps[0])
    arrays = dict(source_latents=z_v.numpy().copy(), source_pano=z_p.numpy().copy(), start_latents=latents.numpy().copy(),
                  start_pano=pano_latent.numpy().copy(), timesteps=np.array(timesteps, dtype=np.int64))
    if masked:
        arrays.update(known_mask=m_v.numpy().copy(), known_pano_mask=m_p.numpy().copy())
    x0_v = x0_p = None
    traj_v, traj_p = [], []
    total = 0.0
    t0 = time.time()
    with torch.no_grad(), FX.chunked_attention():
        for j, t in enumerate(timesteps):
            # PanFusion.py:149: roll the panorama -- and its source, mask, noise and x0 history -- before the call
            pano_latent, cams = oddim.rotate_latent(pano_latent, cams, rot_diff)
            z_p, m_p, n_p = rotate(z_p, rot_diff), rotate(m_p, rot_diff), rotate(n_p, rot_diff)
            x0_p = None if x0_p is None else rotate(x0_p, rot_diff)
            total += rot_diff
            timestep = torch.full((1, m), t, dtype=torch.long)
            eps, pano_eps = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano_latent), oddim.cfg_pair(timestep),
                                  pe, ppe, oddim.cfg_pair(cams))
            eps, pano_eps = oddim.cfg_merge(eps, guidance_scale), oddim.cfg_merge(pano_eps, guidance_scale)
            if solver is None:
                latents, pano_latent = ddim.step(eps, t, latents), ddim.step(pano_eps, t, pano_latent)
            else:
                latents, x0_v = solver.step(eps, i0 + j, latents, x0_v)
                pano_latent, x0_p = solver.step(pano_eps, i0 + j, pano_latent, x0_p)
            if masked:                                       # StableDiffusionInpaintPipeline, num_channels_unet == 4
                last = j == len(timesteps) - 1
                proper_v = z_v if last else add_noise(ddim, z_v, n_v, timesteps[j + 1])
                proper_p = z_p if last else add_noise(ddim, z_p, n_p, timesteps[j + 1])
                latents = (1 - m_v) * proper_v + m_v * latents
                pano_latent = (1 - m_p) * proper_p + m_p * pano_latent
            traj_v.append(latents.numpy().copy())
            traj_p.append(rotate(pano_latent, -total).numpy().copy())           # un-rotated frame
            print("%s step %d t=%d order %s  %.0f s" % (name, j + 1, t, solver.order(i0 + j) if solver else "-", time.time() - t0),
                  flush=True)
    FX.save_golden(os.path.join(OUT, name + ".npz"), latents=np.stack(traj_v), pano_latent=np.stack(traj_p), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("PF_THREADS", os.cpu_count() or 8)))
    model = FX.build_full_width()
    if os.environ.get("PF_GOLDEN_PORT", "0") != "1":
        model = FX.reference_denoiser(model)
        print("cfg1 strength: denoiser =", type(model).__module__, type(model).__name__, flush=True)
    run("cfg1_strength06_ddim10", model, "ddim", masked=False)
    run("cfg1_strength06_inpaint_dpmpp10", model, "dpmpp_2m", masked=True)
    print("done", flush=True)
