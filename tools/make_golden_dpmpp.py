"""Golden trajectory of the DPM-Solver++(2M) sampler at cfg 1 (tests/test_gpu_dpmpp.py).

Runs in the build container (CPU, about a minute per step):

    python tools/make_golden_dpmpp.py

  -> tests/golden/cfg1_dpmpp2m10.npz   configs[0] set-up of tools/make_golden_cfg.py:cfg1 -- m = 4 horizon views of 32x32
                                       latents, 64x128 panorama latent, SD-2-base widths, the REFERENCE's own class as the
                                       denoiser, guidance 9, 90-degree rotation per step -- sampled with 10 steps of 2M
                                       instead of DDIM; latents after every step, panorama in the un-rotated frame.

The solver is written out here in diffusers' own form (DPMSolverMultistepScheduler, algorithm_type="dpmsolver++",
solver_order=2, lower_order_final=True: ``dpm_solver_first_order_update`` / ``multistep_dpm_solver_second_order_update``,
midpoint), in fp32 like oracle/ddim.py, on the DDIM timestep grid the loop uses (leading spacing, steps_offset 1,
prev = t - 1000 // n, the last step targets alphas_cumprod[0]).  It is NOT the kernel's algebra
(DDIM(x, eps) + k (x0 - x0_prev)): the fixture pins that rewrite to the published update.

The panorama's x0 history is rolled together with the latent before each denoiser call (PanFusion.py:149,
PanoGenerator.py:264-269), so that x0 and x0_prev are in the same frame.  The views never roll.
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


class DPMSolverPP2M:
    """diffusers DPMSolverMultistepScheduler(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint",
    lower_order_final=True) restated on oracle.ddim.DDIM's grid and alphas_cumprod; fp32 throughout."""

    def __init__(self, n):
        self.ddim = oddim.DDIM()
        self.timesteps = [int(t) for t in self.ddim.set_timesteps(n)]
        self.n = n

    def alpha_sigma(self, t):
        a = self.ddim.alphas_cumprod[t] if t >= 0 else self.ddim.final_alpha_cumprod
        return a ** 0.5, (1 - a) ** 0.5

    def lam(self, t):
        a, s = self.alpha_sigma(t)
        return torch.log(a) - torch.log(s)

    def order(self, i):
        lower_final = i == self.n - 1 and self.n < 15
        return 1 if (i == 0 or lower_final) else 2

    def step(self, eps, i, sample, x0_prev):
        """One update from timesteps[i]; returns (x_t, x0).  x0_prev: the previous step's x0 in this step's frame."""
        s0 = self.timesteps[i]
        t = s0 - self.ddim.num_train_timesteps // self.n
        alpha_s0, sigma_s0 = self.alpha_sigma(s0)
        alpha_t, sigma_t = self.alpha_sigma(t)
        x0 = (sample - sigma_s0 * eps) / alpha_s0                 # convert_model_output, epsilon prediction
        h = self.lam(t) - self.lam(s0)
        if self.order(i) == 1:                                     # dpm_solver_first_order_update
            return (sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * x0, x0
        s1 = self.timesteps[i - 1]
        r0 = (self.lam(s0) - self.lam(s1)) / h
        D0, D1 = x0, (1.0 / r0) * (x0 - x0_prev)
        x_t = ((sigma_t / sigma_s0) * sample - (alpha_t * (torch.exp(-h) - 1.0)) * D0
               - 0.5 * (alpha_t * (torch.exp(-h) - 1.0)) * D1)
        return x_t, x0


def rotate(x, degree):
    return torch.roll(x, int(degree / 360 * x.shape[-1]), dims=-1) if degree % 360 else x


def cfg1_dpmpp2m10(steps=10, rot_diff=90.0, guidance_scale=9.0):
    model = FX.build_full_width()
    if os.environ.get("PF_GOLDEN_PORT", "0") != "1":
        model = FX.reference_denoiser(model)
        print("cfg1 2M: denoiser =", type(model).__module__, type(model).__name__, flush=True)
    cams = FX.horizon4_cameras()
    latents, pano_latent, pe, ppe = FX.loop_inputs(cams, (32, 32), (64, 128))
    m = latents.shape[1]
    sched = DPMSolverPP2M(steps)
    x0_v = x0_p = None
    traj_v, traj_p = [], []
    total = 0.0
    t0 = time.time()
    with torch.no_grad(), FX.chunked_attention():
        for i, t in enumerate(sched.timesteps):
            # PanFusion.py:149: roll the panorama (and, here, its x0 history) before the call
            pano_latent, cams = oddim.rotate_latent(pano_latent, cams, rot_diff)
            if x0_p is not None:
                x0_p = rotate(x0_p, rot_diff)
            total += rot_diff
            timestep = torch.full((1, m), t, dtype=torch.long)
            eps, pano_eps = model(oddim.cfg_pair(latents), oddim.cfg_pair(pano_latent), oddim.cfg_pair(timestep),
                                  pe, ppe, oddim.cfg_pair(cams))
            eps, pano_eps = oddim.cfg_merge(eps, guidance_scale), oddim.cfg_merge(pano_eps, guidance_scale)
            latents, x0_v = sched.step(eps, i, latents, x0_v)
            pano_latent, x0_p = sched.step(pano_eps, i, pano_latent, x0_p)
            traj_v.append(latents.numpy().copy())
            traj_p.append(rotate(pano_latent, -total).numpy().copy())           # un-rotated frame
            print("cfg1 2M step %d t=%d order %d  %.0f s" % (i + 1, t, sched.order(i), time.time() - t0), flush=True)
    FX.save_golden(os.path.join(OUT, "cfg1_dpmpp2m10.npz"), latents=np.stack(traj_v), pano_latent=np.stack(traj_p),
                   timesteps=np.array(sched.timesteps, dtype=np.int64))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("PF_THREADS", os.cpu_count() or 8)))
    cfg1_dpmpp2m10()
    print("done", flush=True)
