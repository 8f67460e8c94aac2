"""The DDIM sampling loop around the denoiser (reference
``models/pano/PanFusion.py:30-43,100-164``, ``PanoGenerator.py:240-269``).

``DenoiseLoop`` owns the static device buffers of one sampling run and runs
one loop iteration -- 90-degree latent roll, CFG-paired dual-branch denoiser,
CFG merge, two DDIM updates -- per ``step()``.  The denoiser call can be
captured into one hipGraph per rotation offset (the geometry is 4-periodic,
SURVEY.md §4) and replayed; the CFG+DDIM update is a separate fused kernel
whose scalar coefficients change every step.  ``sampler="dpmpp_2m"`` swaps the
update for DPM-Solver++(2M) on the same timestep grid (``DPMSolverSchedule``,
DESIGN.md §4.5); DDIM stays the default.  ``known=KnownRegion(...)`` blends
known content into the state inside the same two update launches
(inpainting / outpainting).  ``strength=s, init=SourceLatents(...)``
starts from a noised source and runs the last ``int(steps * s)`` steps of the grid
(image-to-panorama, partial-strength inpainting), and ``restart()`` re-arms a loop
in place -- same buffers, same captured graphs -- for the next run.
``SourceLatents(..., resample="bicubic")`` admits a source smaller than the loop by integer factors, up-sampled inside the
start launch (periodic in longitude for the panorama), and ``HiResLoop`` chains a base pass and a refine pass at a larger
size on one model: two-pass high-resolution sampling.
"""
import copy
import math
import os

import torch

from . import ops
from .external.Perspective_and_Equirectangular import e2p


class DDIMSchedule:
    """diffusers DDIMScheduler with the SD-2-base config (scaled-linear betas 0.00085..0.012,
    1000 train steps, steps_offset 1, leading spacing, eta 0, epsilon prediction)."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.num_train_timesteps, self.steps_offset = num_train_timesteps, steps_offset

    def set_timesteps(self, n):
        self.num_inference_steps = n
        ratio = self.num_train_timesteps // n
        self.timesteps = [int(i * ratio) + self.steps_offset for i in range(n)][::-1]
        return self.timesteps

    def coefficients(self, t):
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        return (float(a_t ** 0.5), float((1 - a_t) ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))


class DPMSolverSchedule:
    """DPM-Solver++(2M) (diffusers DPMSolverMultistepScheduler, algorithm_type="dpmsolver++", solver_type="midpoint") on
    DDIMSchedule's grid and alphas_cumprod: leading spacing, steps_offset 1, the target of step t is t - 1000 // n, the last
    step targets alphas_cumprod[0] (set_alpha_to_one=False).

    With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log alpha - log sigma, s0 = timesteps[i], t = its target and
    s1 = timesteps[i - 1], diffusers' second-order update
        x_t = (sigma_t / sigma_s0) x - alpha_t (e^-h - 1) D0 - 1/2 alpha_t (e^-h - 1) D1,  D0 = x0, D1 = (x0 - x0_prev) / r0,
        h = lambda_t - lambda_s0,  r0 = (lambda_s0 - lambda_s1) / h
    is DDIM(x, eps) (its first two terms) + k (x0 - x0_prev) with k = 1/2 alpha_t (1 - e^-h) / r0.  ``step_coefficients(i)``
    gives the DDIM 4-tuple (bit for bit DDIMSchedule's), k (float64) and the order: 1 at the first step, at the last one when
    there are fewer than 15 steps (lower_order_final) and everywhere with solver_order=1 (then the loop is the DDIM loop)."""

    def __init__(self, solver_order=2, lower_order_final=True):
        if solver_order not in (1, 2):
            raise ValueError("DPMSolverSchedule: solver_order must be 1 or 2, got %r" % (solver_order,))
        self.solver_order, self.lower_order_final = solver_order, bool(lower_order_final)
        self.ddim = DDIMSchedule()
        self.alphas_cumprod, self.final_alpha_cumprod = self.ddim.alphas_cumprod, self.ddim.final_alpha_cumprod
        self.num_train_timesteps = self.ddim.num_train_timesteps

    def set_timesteps(self, n):
        self.timesteps = self.ddim.set_timesteps(n)
        self.num_inference_steps = n
        return self.timesteps

    def alpha_sigma(self, t):
        """(alpha, sigma) of timestep t in float64; t < 0 is the final target alphas_cumprod[0]."""
        a = float(self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod)
        return math.sqrt(a), math.sqrt(1.0 - a)

    def lam(self, t):
        a, s = self.alpha_sigma(t)
        return math.log(a) - math.log(s)

    def prev(self, t):
        return t - self.num_train_timesteps // self.num_inference_steps

    def order(self, i, first=False):
        n = len(self.timesteps)
        if self.solver_order == 1 or i == 0 or first or (self.lower_order_final and i == n - 1 and n < 15):
            return 1
        return 2

    def step_coefficients(self, i, first=False):
        """(DDIM 4-tuple, k, order) of step index i; k = 0.0 at a first-order step.  ``first``: i is the first step a run
        executes (a strength < 1 start): no history yet, so first order whatever i is (diffusers'
        lower_order_nums < 1); lower_order_final keeps looking at the full grid."""
        s0 = self.timesteps[i]
        coef = self.ddim.coefficients(s0)
        order = self.order(i, first)
        if order == 1:
            return coef, 0.0, 1
        t, s1 = self.prev(s0), self.timesteps[i - 1]
        lam_t, lam_s0, lam_s1 = self.lam(t), self.lam(s0), self.lam(s1)
        h = lam_t - lam_s0
        r0 = (lam_s0 - lam_s1) / h
        k = 0.5 * self.alpha_sigma(t)[0] * -math.expm1(-h) / r0
        return coef, k, 2


def _make_sampler(sampler):
    """DenoiseLoop's ``sampler`` argument -> None (DDIM) or a private DPMSolverSchedule."""
    if isinstance(sampler, DPMSolverSchedule):
        return copy.deepcopy(sampler)                   # set_timesteps below must not touch the caller's object
    if isinstance(sampler, str) and sampler == "ddim":
        return None
    if isinstance(sampler, str) and sampler == "dpmpp_2m":
        return DPMSolverSchedule()
    raise ValueError("sampler must be 'ddim', 'dpmpp_2m' or a DPMSolverSchedule, got %r" % (sampler,))


def init_noise(pano_noise, cameras, pers_h, pers_w):
    """View noise = nearest-neighbour e2p of the SAME panorama noise (PanFusion.py:30-43).
    pano_noise (bs, 1, 4, H, W) on the GPU; cameras: dict of (bs, m)."""
    bs = pano_noise.shape[0]
    m = cameras["FoV"].shape[1]
    flat = {k: v.reshape(-1) for k, v in cameras.items()}
    rep = pano_noise.expand(-1, m, -1, -1, -1).flatten(0, 1)
    noise = e2p(rep, flat["FoV"], flat["theta"], flat["phi"], (pers_h, pers_w), mode="nearest")
    return pano_noise, noise.unflatten(0, (bs, m))


def stitch_views(images, cameras, out_hw, **kw):
    """The perspective branch seen as a panorama: the m views of a run stitched by ``mp2e`` (feathered where they overlap).
    images: the uint8 views (b, m, h, w, 3) that ``vae.decode_views_and_pano`` returns, or a float tensor (b, m, C, h, w), on
    the GPU; cameras: dict of (b, m) (FoV, theta, phi in degrees, as the loops take them); out_hw: the panorama size in
    pixels.  Returns float32 (b, C, H, W) on the scale of the input; ``kw`` (mode, feather, fill, return_weight) goes to mp2e."""
    from .external.Perspective_and_Equirectangular.mp2e import mp2e
    if not isinstance(images, torch.Tensor) or images.dim() != 5:
        raise ValueError("stitch_views: images (b, m, h, w, 3) uint8 or (b, m, C, h, w) float expected, got %s"
                         % (getattr(images, "shape", type(images)),))
    if images.dtype == torch.uint8:
        images = images.permute(0, 1, 4, 2, 3).float()
    want = tuple(images.shape[:2])
    for k in ("FoV", "theta", "phi"):
        if tuple(cameras[k].shape) != want:
            raise ValueError("stitch_views: cameras[%r] must be %s, got %s" % (k, want, tuple(cameras[k].shape)))
    return mp2e(images, cameras["FoV"].reshape(-1), cameras["theta"].reshape(-1), cameras["phi"].reshape(-1), out_hw, **kw)


def faed(real_panos, generated_panos, metric):
    """The Fréchet Auto-Encoder Distance between two sets of panoramas ([N, 3, H, W], uint8 or float on the 0..255 scale, at least two
    each; a list of such batches is taken batch by batch) through ``metric``, a ``models.faed.FrechetAutoEncoderDistance``.  The
    metric is reset first and keeps the accumulated states afterwards (``merge`` them across ranks before ``compute``)."""
    metric.reset()
    for panos, real in ((real_panos, True), (generated_panos, False)):
        for batch in ([panos] if isinstance(panos, torch.Tensor) else panos):
            metric.update(batch, real)
    return metric.compute()


def _keep_mask(gen):
    """An image-resolution mask (n, 1, 8h, 8w), 1 = generate -> the latent mask (n, 1, h, w): a latent pixel is kept (0) only
    if all 64 pixels of its 8x8 block are known (mask < 0.5, diffusers' binarisation)."""
    return torch.nn.functional.max_pool2d((gen >= 0.5).float(), 8)


def _encode_panorama(vae_encoder, pano, cameras, view_hw, latent_pad=8):
    """(view latents (1, m, 4, h, w), panorama latent (1, 1, 4, H, W)) of a panorama (1, 1, 3, Hp, Wp) in [-1, 1]: the VAE
    posterior mean x scaling_factor of the circularly padded panorama, unpadded (as the training step encodes it, without the
    sample draw), and the means of its bilinear e2p crops at 8 view_hw."""
    from .utils.pano import pad_pano, unpad_pano
    sf = vae_encoder.packed(pano.device).scaling_factor
    mean, _ = vae_encoder.encode(pad_pano(pano[0].float(), 8 * latent_pad))
    pano_latent = (unpad_pano(mean, latent_pad) * sf).contiguous()[None]
    m = cameras["FoV"].shape[1]
    flat = {k: v.reshape(-1) for k, v in cameras.items()}
    hw = (8 * view_hw[0], 8 * view_hw[1])
    crops = e2p(pano[0].float().expand(m, -1, -1, -1), flat["FoV"], flat["theta"], flat["phi"], hw, mode="bilinear")
    latents = (vae_encoder.encode(crops)[0] * sf)[None]
    return latents, pano_latent


def _check_shapes(what, named, batch):
    """ValueError unless the loop's latents have batch 1 and every (name, tensor, shape) of ``named`` fits."""
    lat, pano = batch
    if lat[0] != 1 or pano[0] != 1:
        raise ValueError("%s: batch 1 only, the loop's latents are %s / %s" % (what, lat, pano))
    for name, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %s, got %s" % (what, name, shape, getattr(t, "shape", type(t))))


RESAMPLE_MODES = ("nearest", "bilinear", "bicubic")


class SourceLatents:
    """The clean source latents z of a strength < 1 run: latents (1, m, 4, h, w) for the views and pano_latent
    (1, 1, 4, H, W) for the panorama, in the caller's (un-rotated) frame.  ``DenoiseLoop(..., strength=s, init=...)`` starts
    from add_noise(z, noise, t_s) and checks the shapes against its latents.
    ``resample`` ("nearest", "bilinear" or "bicubic"): the source may be SMALLER than the loop's latents by integer
    factors, views and panorama independently; the start launch up-samples it with torch's interpolate semantics
    (align_corners=False), the panorama periodic in longitude, the views clamped.  None: the shapes must be equal."""

    def __init__(self, latents, pano_latent, resample=None):
        if resample is not None and resample not in RESAMPLE_MODES:
            raise ValueError("SourceLatents: resample must be None or one of %s, got %r" % (RESAMPLE_MODES, resample))
        self.latents, self.pano_latent, self.resample = latents, pano_latent, resample

    @classmethod
    def from_panorama(cls, vae_encoder, pano, cameras, view_hw, latent_pad=8):
        """Encode a panorama (1, 1, 3, Hp, Wp) in [-1, 1] on the GPU exactly as KnownRegion.from_panorama does; cameras: dict of
        (1, m) (FoV, theta, phi in degrees, as DenoiseLoop takes them); view_hw: the view LATENT size."""
        if pano.dim() != 5 or pano.shape[:3] != (1, 1, 3):
            raise ValueError("SourceLatents.from_panorama: pano (1, 1, 3, Hp, Wp) expected, got %s" % (tuple(pano.shape),))
        return cls(*_encode_panorama(vae_encoder, pano, cameras, view_hw, latent_pad))

    def check(self, latents, pano_latent):
        """ValueError unless the source fits the loop's latents (batch 1): equal shapes, or -- with ``resample`` -- equal
        leading dimensions and a height and width that divide the loop's."""
        lat, pano = tuple(latents.shape), tuple(pano_latent.shape)
        if self.resample is None:
            _check_shapes("source latents", (("latents", self.latents, lat), ("pano_latent", self.pano_latent, pano)), (lat, pano))
            return
        _check_shapes("source latents", (), (lat, pano))
        for name, t, shape in (("latents", self.latents, lat), ("pano_latent", self.pano_latent, pano)):
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else None
            if got is None or len(got) != len(shape) or got[:-2] != shape[:-2] or min(got[-2:]) < 1 \
                    or shape[-2] % got[-2] or shape[-1] % got[-1]:
                raise ValueError("source latents: %s must be %s or smaller by integer factors in height and width (resample=%r), "
                                 "got %s" % (name, shape, self.resample, getattr(t, "shape", type(t))))


def executed_steps(steps, strength):
    """(k, i0) of a strength-s run on a grid of ``steps``: k = min(int(steps * s), steps) executed steps starting at grid index
    i0 = steps - k (get_timesteps of diffusers' img2img / inpaint pipelines, Python's int() of the float product exactly).
    ValueError for a strength outside (0, 1], NaN, or one that leaves no step."""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0 < strength <= 1:
        raise ValueError("strength must be a number in (0, 1], got %r" % (strength,))
    k = min(int(steps * strength), steps)
    if k == 0:
        raise ValueError("strength %r leaves no step to run on a grid of %d (int(steps * strength) == 0)" % (strength, steps))
    return k, steps - k


class KnownRegion:
    """Latent-level known content of an inpainting / outpainting run.

    latents (1, m, 4, h, w) and mask (1, m, 1, h, w) for the views, pano_latent (1, 1, 4, H, W) and pano_mask (1, 1, 1, H, W) for
    the panorama, all in the caller's (un-rotated) frame.  MASK CONVENTION (diffusers'): 1 = generate, 0 = keep, values in
    [0, 1].  ``DenoiseLoop(..., known=...)`` checks the shapes against its latents."""

    def __init__(self, latents, mask, pano_latent, pano_mask):
        self.latents, self.mask, self.pano_latent, self.pano_mask = latents, mask, pano_latent, pano_mask

    @classmethod
    def from_panorama(cls, vae_encoder, pano, pano_mask, cameras, view_hw, latent_pad=8):
        """Encode a (partly) known panorama.  pano (1, 1, 3, Hp, Wp) in [-1, 1] and pano_mask (1, 1, 1, Hp, Wp), 1 = generate, on
        the GPU; cameras: dict of (1, m) (FoV, theta, phi in degrees, as DenoiseLoop takes them); view_hw: the view LATENT size.
        The panorama latent is the VAE posterior mean x scaling_factor of the circularly padded panorama, unpadded (as the
        training step encodes it, without the sample draw); the view latents are the means of its bilinear e2p crops at
        8 view_hw.  A latent pixel is kept only if all 64 pixels of its 8x8 block are known: in pano_mask for the panorama, in
        each view's nearest e2p crop of pano_mask for that view."""
        if pano.shape[:3] != (1, 1, 3) or pano_mask.shape != (1, 1, 1) + tuple(pano.shape[-2:]):
            raise ValueError("KnownRegion.from_panorama: pano (1, 1, 3, Hp, Wp) and pano_mask (1, 1, 1, Hp, Wp) expected, got %s, %s"
                             % (tuple(pano.shape), tuple(pano_mask.shape)))
        latents, pano_latent = _encode_panorama(vae_encoder, pano, cameras, view_hw, latent_pad)
        m = cameras["FoV"].shape[1]
        flat = {k: v.reshape(-1) for k, v in cameras.items()}
        hw = (8 * view_hw[0], 8 * view_hw[1])
        mask_crops = e2p(pano_mask[0].float().expand(m, -1, -1, -1), flat["FoV"], flat["theta"], flat["phi"], hw, mode="nearest")
        return cls(latents, _keep_mask(mask_crops)[None], pano_latent, _keep_mask(pano_mask[0].float())[None])

    @classmethod
    def from_view(cls, vae_encoder, image, fov, theta, phi, cameras, pano_hw, view_hw):
        """Outpaint one photo to 360 degrees: image (1, 3, hi, wi) in [-1, 1] on the GPU, seen with horizontal field of view
        ``fov`` at (theta, phi) degrees, is projected (p2e) into a panorama of 8 pano_hw pixels, the pixels it does not cover set
        to 0 and generated (the p2e mask); then from_panorama.  pano_hw / view_hw: the panorama / view LATENT sizes."""
        from .external.Perspective_and_Equirectangular.p2e import p2e
        if image.dim() != 4 or image.shape[:2] != (1, 3):
            raise ValueError("KnownRegion.from_view: image (1, 3, h, w) expected, got %s" % (tuple(image.shape),))
        equi, covered = p2e(image.float(), [fov], [theta], [phi], (8 * pano_hw[0], 8 * pano_hw[1]))
        pano = torch.where(covered, equi, torch.zeros((), device=equi.device))
        return cls.from_panorama(vae_encoder, pano[None], (~covered).float()[None], cameras, view_hw)

    @classmethod
    def from_views(cls, vae_encoder, images, fovs, thetas, phis, cameras, pano_hw, view_hw, feather="both"):
        """Outpaint from several photos: images (n, 3, hi, wi) in [-1, 1] on the GPU, photo i seen with horizontal field of view
        fovs[i] at (thetas[i], phis[i]) degrees, are stitched (mp2e, bilinear, fill 0) into a panorama of 8 pano_hw pixels,
        feathered where they overlap; the pixels that no photo covers with positive weight are generated; then from_panorama.
        pano_hw / view_hw: the panorama / view LATENT sizes.  The feather tent is 0 on a photo's outermost columns (and rows,
        with feather="both"), so one photo through from_views covers slightly less than the same photo through from_view."""
        from .external.Perspective_and_Equirectangular.mp2e import mp2e
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError("KnownRegion.from_views: images (n, 3, h, w) expected, got %s" % (getattr(images, "shape", type(images)),))
        n = images.shape[0]
        if not len(fovs) == len(thetas) == len(phis) == n:
            raise ValueError("KnownRegion.from_views: %d images need %d cameras, got %d / %d / %d"
                             % (n, n, len(fovs), len(thetas), len(phis)))
        pano, weight = mp2e(images.float(), fovs, thetas, phis, (8 * pano_hw[0], 8 * pano_hw[1]), "bilinear", feather=feather,
                            fill=0.0, return_weight=True)
        return cls.from_panorama(vae_encoder, pano[None, None], (weight == 0).float()[None, None], cameras, view_hw)

    def check(self, latents, pano_latent):
        """ValueError unless the known content fits the loop's latents (batch 1) and the masks lie in [0, 1]."""
        lat, pano = tuple(latents.shape), tuple(pano_latent.shape)
        if lat[0] != 1 or pano[0] != 1:
            raise ValueError("known content: batch 1 only, the loop's latents are %s / %s" % (lat, pano))
        want = ((self.latents, lat), (self.mask, lat[:2] + (1,) + lat[3:]), (self.pano_latent, pano),
                (self.pano_mask, pano[:2] + (1,) + pano[3:]))
        for name, (t, shape) in zip(("latents", "mask", "pano_latent", "pano_mask"), want):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError("known content: %s must be %s, got %s" % (name, shape, getattr(t, "shape", type(t))))
        for name, t in (("mask", self.mask), ("pano_mask", self.pano_mask)):
            if not bool(((t >= 0) & (t <= 1)).all()):
                raise ValueError("known content: %s values must lie in [0, 1] (1 = generate, 0 = keep)" % name)


def rotate_cameras(cameras, degree):
    cams = dict(cameras)
    cams["theta"] = (cams["theta"] + degree) % 360
    return cams


class DenoiseLoop:
    """One sampling run (batch 1 prompt, CFG pair inside): text-to-panorama from noise, with ``known`` content kept
    (inpainting / outpainting), and / or from a noised source at ``strength`` < 1 (``init``); ``restart()`` re-arms it in
    place for the next run."""

    def __init__(self, model, latents, pano_latent, prompt_embd, pano_prompt_embd, cameras,
                 steps=50, rot_diff=90.0, guidance_scale=9.0, use_graphs=False, pano_layout_cond=None, sampler="ddim",
                 known=None, strength=1.0, init=None, guidance_rescale=0.0):
        """latents (1, m, 4, h, w), pano_latent (1, 1, 4, H, W) fp32 on the GPU: the NOISE (init_noise);
        prompt_embd (2, m, L, D) / pano_prompt_embd (2, 1, L, D) = [null ; prompt];
        cameras: dict of (1, m) CPU tensors (FoV, theta, phi in degrees);
        sampler: "ddim" (default), "dpmpp_2m" or a DPMSolverSchedule (changes the outputs by design: DESIGN.md §4.5);
        known: a KnownRegion -- inpainting / outpainting;
        strength in (0, 1], init: a SourceLatents -- the run starts from add_noise(init, noise, t_s) and executes the last
        int(steps * strength) steps of the grid; init defaults to the known latents.  At strength 1 the start
        is the noise itself, with or without init.
        guidance_rescale in [0, 1]: diffusers' ``guidance_rescale`` (rescale_noise_cfg), phi of DESIGN.md §4.9 -- the guided
        prediction is scaled per latent towards the spread of the conditional one; 0 (default) is the loop without it."""
        k, i0 = executed_steps(steps, strength)
        if not (isinstance(guidance_rescale, (int, float)) and 0.0 <= guidance_rescale <= 1.0):
            raise ValueError("guidance_rescale %r must be a number in [0, 1]" % (guidance_rescale,))
        if known is not None:
            known.check(latents, pano_latent)
        if init is not None:
            init.check(latents, pano_latent)
        if k < steps:
            if init is None and known is None:
                raise ValueError("strength %r < 1 needs source latents: init=SourceLatents(...) or known=KnownRegion(...)" % (strength,))
            if latents.shape[0] != 1 or pano_latent.shape[0] != 1:
                raise ValueError("strength < 1: batch 1 only, the loop's latents are %s / %s"
                                 % (tuple(latents.shape), tuple(pano_latent.shape)))
        self.model, self.guidance, self.rot_diff = model, guidance_scale, rot_diff
        self.prompt, self.pano_prompt = prompt_embd, pano_prompt_embd
        self._cameras0 = {k_: v.detach().cpu() for k_, v in cameras.items()}
        self.m = latents.shape[1]
        self.W = pano_latent.shape[-1]
        self.shift = int(rot_diff / 360 * self.W)          # PanoGenerator.py:269
        self.sched = DDIMSchedule()
        self.steps = steps
        self._grid = self.sched.set_timesteps(steps)
        self.strength, self.i0 = strength, i0
        self.timesteps = self._grid[i0:]                   # the executed steps (all of the grid at strength 1)
        self.solver = _make_sampler(sampler)
        dev = latents.device
        own = lambda t: t.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
        # The loop's state lives as the CFG PAIR the denoiser reads ([x ; x], gen_cls_free_guide_pair, PanoGenerator.py:240-251):
        # the DDIM kernel writes both halves, so no torch.cat runs between two calls.  self.lat / self.pano are the first halves.
        if k == steps:
            self.lat2 = torch.stack([latents.float()[0]] * 2).contiguous()
            self.pano2 = torch.stack([pano_latent.float()[0]] * 2).contiguous()
        else:                                              # filled by _write_start below
            self.lat2 = torch.empty((2,) + tuple(latents.shape[1:]), dtype=torch.float32, device=dev)
            self.pano2 = torch.empty((2,) + tuple(pano_latent.shape[1:]), dtype=torch.float32, device=dev)
        self.known = known
        if known is not None:
            # fp32 operands of the blend, all in the caller's frame (the kernel reads the panorama's at the state's offset): the
            # known latents, the masks expanded over the 4 channels, and the noise n, before the first roll
            self.known_lat, self.known_pano = own(known.latents), own(known.pano_latent)
            self.mask_lat, self.mask_pano = own(known.mask.expand_as(latents)), own(known.pano_mask.expand_as(pano_latent))
        # the noise operand: the loop's own copy where a kernel reads it after construction (the blend; restart() copies new
        # noise into it), the caller's tensors otherwise until a restart() needs them
        self._owns_noise = known is not None or k < steps
        self.noise_lat, self.noise_pano = (own(latents), own(pano_latent)) if self._owns_noise else (latents, pano_latent)
        # the source z of a strength < 1 start: the loop's own copy of init, else the known latents themselves
        # (its own size with init.resample: the start kernel up-samples it)
        self.src_lat = self.src_pano = self.resample = None
        if init is not None:
            self.src_lat, self.src_pano, self.resample = own(init.latents), own(init.pano_latent), init.resample
        self.tstep = torch.empty(2, self.m, dtype=torch.long, device=dev)
        self.rescale = float(guidance_rescale)
        self.rescale_factors = None
        if self.rescale > 0:
            # per-latent float64 partial sums of the two predictions (ops.cfg_moments) and the factors f of the last step
            # (views, panorama): allocated here, written by the two extra launches of every step, never read by the host
            self._moments_lat = torch.empty(1, ops.CFG_PARTIALS, ops.CFG_MOMENT_DOUBLES, dtype=torch.float64, device=dev)
            self._moments_pano = torch.empty_like(self._moments_lat)
            self.rescale_factors = torch.ones(2, dtype=torch.float32, device=dev)
        self.use_graphs = use_graphs
        self.graphs = {}
        # layout condition image (1, 1, 3, Hi, Wi) for the panorama ControlNet: rolled with the panorama
        # every step (PanFusion.py:150-153); one static copy per rotation offset (the loop is 4-periodic)
        self.layout = None if pano_layout_cond is None else pano_layout_cond.float().contiguous()
        self._layout_rot = {}
        self.eps = self.pano_eps = None
        self._rot_of = {}                                  # camera-theta key -> accumulated rotation (degrees)
        self.lat, self.pano = self.lat2[:1], self.pano2[:1]
        if self.solver is not None:
            self.solver.set_timesteps(steps)
            # the multistep history: x0 of the previous step, one buffer per latent (never shared); the panorama's is kept in the
            # frame of the next call (the update kernel writes it rolled, as it writes the state)
            self.x0_lat = torch.empty_like(self.lat)
            self.x0_pano = torch.empty_like(self.pano)
        # The loop rolls the panorama BEFORE each denoiser call (PanFusion.py:149); afterwards the DDIM kernel writes the next
        # latent already rolled for the following step.
        if k == steps:
            if rot_diff % 360:
                self.pano2.copy_(ops.roll_width(self.pano2, self.shift))       # (one-off set-up, not part of a step)
            self._tstep_value = None                      # what self.tstep holds (the DDIM kernel writes the next step's value)
        else:
            self._write_start()
        self._rewind()

    def _rewind(self):
        """Counters and cameras of "constructed, before the first step": the state has been rolled once."""
        self.i = 0                                         # EXECUTED steps so far; the grid index of a step is i0 + i
        self.cameras = rotate_cameras(self._cameras0, self.rot_diff)
        self.total_rot = 0.0 + self.rot_diff
        self._rot_of.setdefault(tuple(float(v) for v in self.cameras["theta"].reshape(-1)), self.total_rot)

    def _write_start(self):
        """The start state, both halves of the pair, rolled for the first call, and the first call's timestep words, written IN
        PLACE by two launches (captured graphs read these buffers): add_noise(z, n, t_s) below strength 1, n itself at 1."""
        t0 = self.timesteps[0]
        ka = kb = 0.0
        z_lat = z_pano = None
        if self.i0 > 0:
            ka, kb = self.sched.coefficients(t0)[:2]
            z_lat, z_pano = (self.known_lat, self.known_pano) if self.src_lat is None else (self.src_lat, self.src_pano)
        roll = self.shift if self.rot_diff % 360 else 0
        self._start_launch(z_lat, self.noise_lat, ka, kb, 0, False, out=self.lat, out2=self.lat2[1:])
        self._start_launch(z_pano, self.noise_pano, ka, kb, roll, True, out=self.pano, out2=self.pano2[1:], tstep=self.tstep, t0=t0)
        self._tstep_value = t0

    def _start_launch(self, z, noise, ka, kb, roll, wrap, **out):
        """One start launch: noised_start_pair, or -- for a source smaller than the latent -- the launch that
        up-samples it on the way, periodic in longitude (``wrap``) for the panorama."""
        if z is None or z.shape[-2:] == noise.shape[-2:]:
            ops.noised_start_pair(z, noise, ka, kb, roll, **out)
        else:
            ops.upsampled_start_pair(z, noise, ka, kb, roll, mode=self.resample, wrap=wrap, **out)

    def restart(self, latents=None, pano_latent=None, *, strength=None, init=None, known=None):
        """Back to "constructed, before the first step" IN PLACE: state pair, timestep words, step counters, cameras, total_rot,
        the 2M order; and -- where given -- new noise, a new source, new known contents (same shapes, copied into the loop's own
        operand buffers) and a new strength.  None keeps the current value.  Captured graphs, EPA tables and pinned text K/V stay
        valid: no buffer a graph reads is allocated and no address changes.  A new source may have another admissible size
        (``SourceLatents(..., resample=)``): the source buffers are operands of the start launch only, so they
        are re-allocated then.  Not re-armable: steps, sampler, rot_diff, guidance, guidance_rescale,
        prompts, cameras, and whether the loop has known content at all."""
        shape_lat, shape_pano = (1,) + tuple(self.lat.shape[1:]), (1,) + tuple(self.pano.shape[1:])
        like_lat, like_pano = torch.empty(shape_lat, device="meta"), torch.empty(shape_pano, device="meta")
        _check_shapes("restart", [(n, t, s) for n, t, s in (("latents", latents, shape_lat), ("pano_latent", pano_latent, shape_pano))
                                  if t is not None], (shape_lat, shape_pano))
        if known is not None:
            if self.known is None:
                raise ValueError("restart: this loop was built without known content (known= cannot be added by a restart)")
            known.check(like_lat, like_pano)
        if init is not None:
            init.check(like_lat, like_pano)
        new_strength = self.strength if strength is None else strength
        k, i0 = executed_steps(self.steps, new_strength)
        if k < self.steps and init is None and self.src_lat is None and self.known is None:
            raise ValueError("restart: strength %r < 1 needs source latents: init=SourceLatents(...)" % (new_strength,))
        # everything is valid: from here on the loop changes
        dev = self.lat.device
        put = lambda buf, t: buf.copy_(t.detach().to(dev, torch.float32))
        if not self._owns_noise:
            # a loop built with defaults kept the caller's noise tensors: it takes its own copies now (operands of the start
            # kernel only; no graph reads them)
            own = lambda t: t.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
            self.noise_lat = own(self.noise_lat if latents is None else latents)
            self.noise_pano = own(self.noise_pano if pano_latent is None else pano_latent)
            self._owns_noise, latents, pano_latent = True, None, None
        if latents is not None:
            put(self.noise_lat, latents)
        if pano_latent is not None:
            put(self.noise_pano, pano_latent)
        if known is not None:
            self.known = known
            put(self.known_lat, known.latents)
            put(self.known_pano, known.pano_latent)
            put(self.mask_lat, known.mask.expand_as(self.mask_lat))
            put(self.mask_pano, known.pano_mask.expand_as(self.mask_pano))
        if init is not None:
            own = lambda t: t.detach().to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
            fits = lambda buf, t: buf is not None and buf.shape == t.shape
            self.src_lat = put(self.src_lat, init.latents) if fits(self.src_lat, init.latents) else own(init.latents)
            self.src_pano = put(self.src_pano, init.pano_latent) if fits(self.src_pano, init.pano_latent) else own(init.pano_latent)
            self.resample = init.resample
        self.strength, self.i0 = new_strength, i0
        self.timesteps = self._grid[i0:]
        self._write_start()
        self._rewind()

    def _layout_for(self, cams):
        """The condition image rolled by the rotation these cameras carry (PanoGenerator.py:264-269)."""
        if self.layout is None:
            return None
        rot = float(self._rot_of.get(tuple(float(v) for v in cams["theta"].reshape(-1)), self.total_rot)) % 360
        if rot not in self._layout_rot:
            shift = int(rot / 360 * self.layout.shape[-1])
            img = ops.roll_width(self.layout, shift) if shift else self.layout
            self._layout_rot[rot] = torch.cat([img, img])          # CFG pair (gen_cls_free_guide_pair)
        return self._layout_rot[rot]

    def _denoise(self, cams):
        cams2 = {k: torch.cat([v, v]) for k, v in cams.items()}                 # (host tensors)
        return self.model(self.lat2, self.pano2, self.tstep, self.prompt, self.pano_prompt, cams2,
                          None, self._layout_for(cams))

    def _set_tstep(self, t):
        if self._tstep_value != t:
            self.tstep.fill_(t)
            self._tstep_value = t

    MAX_GRAPHS = 8        # distinct rotation offsets kept as graphs (4 at rot_diff = 90); beyond that: eager launches

    def _denoise_graphed(self, cams):
        key = tuple(float(v) for v in cams["theta"].reshape(-1))
        g = self.graphs.get(key)
        if g is None and len(self.graphs) >= self.MAX_GRAPHS:
            # a rotation step that does not divide 360 never revisits an offset: capturing (and keeping) a graph
            # plus its table set per step would re-capture every step and grow without bound
            return self._denoise(cams)
        if g is None:
            from .engine import EPATables
            with EPATables.pinned():                 # the graph reads its geometry tables by address
                self._denoise(cams)                  # warm-up: builds tables, sets kernel attributes
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                # PF_VIEW_PRIORITY: capture on the caller's (high-priority) stream, so that the view branch = the critical
                # path keeps that priority and the panorama side stream (default priority) only fills what it leaves idle
                cap = torch.cuda.current_stream() if os.environ.get("PF_VIEW_PRIORITY") else None
                with torch.cuda.graph(graph, stream=cap):
                    out = self._denoise(cams)
            g = (graph, out, self._graph_keepalive())
            self.graphs[key] = g
        g[0].replay()
        return g[1]

    def _graph_keepalive(self):
        """Tensors a captured graph reads by address but that live in bounded caches of the model (16-bit prompt
        casts, text K / V^T per UNet): referenced from the graph entry so that an eviction cannot free them under it."""
        import weakref

        class _Pin:                               # lives exactly as long as the graph entry that holds the returned list
            pass
        owner = _Pin()
        keep = [owner, list(getattr(self.model, "_prompt_cache", {}).values())]
        for packed in getattr(self.model, "_packed", {}).values():
            hits = list(getattr(packed, "text_kv_cache", {}).values())
            for hit in hits:
                # a captured graph reads these buffers by address: refold_lora refreshes them IN PLACE for as long as some graph entry
                # is alive (a WeakSet of the entries' tokens: dropping the loop / its graphs un-pins the entry -- ADVICE r5), and
                # Branch.precompute_text_kv does not evict a pinned entry
                hit.setdefault("pins", weakref.WeakSet()).add(owner)
            keep.append(hits)
        return keep

    def prepare(self):
        """Untimed set-up: build the geometry tables (and capture one hipGraph) for every rotation
        offset the loop will visit (4 at rot_diff = 90)."""
        cams, seen = self.cameras, set()
        self._set_tstep(self.timesteps[0])
        rot = self.total_rot
        for _ in range(64):
            key = tuple(float(v) for v in cams["theta"].reshape(-1))
            if key in seen:
                break
            seen.add(key)
            self._rot_of.setdefault(key, rot)
            rot += self.rot_diff
            (self._denoise_graphed if self.use_graphs else self._denoise)(cams)
            cams = rotate_cameras(cams, self.rot_diff)
        torch.cuda.synchronize()

    def step_eager(self):
        keep, self.use_graphs = self.use_graphs, False
        try:
            self.step()
        finally:
            self.use_graphs = keep

    def step(self):
        """One iteration of the loop body (PanFusion.py:146-162)."""
        t = self.timesteps[self.i]
        self._set_tstep(t)                                # (a no-op after the first step: the DDIM kernel left it there)
        run = self._denoise_graphed if self.use_graphs else self._denoise
        eps, pano_eps = run(self.cameras)
        coef = self.sched.coefficients(t)
        last = self.i == len(self.timesteps) - 1
        # Two launches update the whole loop state IN PLACE (captured graphs read it by address): views -- plain update, both
        # halves of the CFG pair; panorama -- update + roll for the next iteration (a block owns whole rows, so in place for any
        # roll), both halves, and the next call's timestep words.
        t_next = t if last else self.timesteps[self.i + 1]
        self._update(eps, pano_eps, coef, last, t_next)
        self._tstep_value = t_next
        self.i += 1
        if not last:
            self.cameras = rotate_cameras(self.cameras, self.rot_diff)
            self.total_rot += self.rot_diff
            self._rot_of.setdefault(tuple(float(v) for v in self.cameras["theta"].reshape(-1)), self.total_rot)

    def _update(self, eps, pano_eps, coef, last, t_next):
        """The two launches of step() in every mode; each feature adds its keywords once, per latent.
        A solver: the 2M correction, each launch writes its latent's x0 history (the panorama's rolled like the state).
        Known content: the blend after the DDIM or 2M update, x <- m x + (1 - m) r, r = add_noise(known, noise,
        t_next) = ka known + kb noise, known itself at the last step.  On this grid t_next is the DDIM target of the step, so
        (ka, kb) are the step's own (sqrt_a_prev, sqrt_1m_a_prev).  The panorama's operands are read at the offset its state has
        been rolled by before this update: (i + 1) shifts, i counting EXECUTED steps (not total_rot, see result()).
        guidance_rescale > 0: per latent one more launch before the update, for the moments of eps_cond and of
        the guided prediction; the update runs on f eps_cfg and f stays on the device (rescale_factors: views, panorama)."""
        lat, pano = {}, {}
        op = ops.cfg_ddim_step_pair
        if self.solver is not None:
            op = ops.cfg_dpmpp_step_pair
            coef, k, order = self.solver.step_coefficients(self.i0 + self.i, first=self.i == 0)
            lat.update(x0_prev=self.x0_lat if order == 2 else None, k=k, x0_out=self.x0_lat)
            pano.update(x0_prev=self.x0_pano if order == 2 else None, k=k, x0_out=self.x0_pano)
        if self.known is not None:
            op = ops.cfg_inpaint_step_pair
            ka, kb = (1.0, 0.0) if last else coef[2:]
            o = (self.i + 1) * self.shift % self.W
            lat.update(known=self.known_lat, noise=self.noise_lat, mask=self.mask_lat, ka=ka, kb=kb, known_roll=0)
            pano.update(known=self.known_pano, noise=self.noise_pano, mask=self.mask_pano, ka=ka, kb=kb, known_roll=o)
        if self.rescale > 0:
            op = ops.cfg_rescaled_step_pair
            lat.update(partials=self._moments_lat, phi=self.rescale, factor_out=self.rescale_factors[:1])
            pano.update(partials=self._moments_pano, phi=self.rescale, factor_out=self.rescale_factors[1:])
            ops.cfg_moments(eps[0], eps[1], self.guidance, samples=1, out=self._moments_lat)
        op(self.lat, eps[0], eps[1], self.guidance, coef, 0, out=self.lat, out2=self.lat2[1:], **lat)
        if self.rescale > 0:
            ops.cfg_moments(pano_eps[0], pano_eps[1], self.guidance, samples=1, out=self._moments_pano)
        op(self.pano, pano_eps[0], pano_eps[1], self.guidance, coef, 0 if last else self.shift, out=self.pano, out2=self.pano2[1:],
           tstep=self.tstep, t_next=t_next, **pano)

    def run(self):
        while self.i < len(self.timesteps):
            self.step()
        return self.result()

    def result(self):
        """Latents with the accumulated rotation undone (PanFusion.py:164)."""
        back = int(-self.total_rot / 360 * self.W)
        return self.lat, ops.roll_width(self.pano, back)


class HiResLoop:
    """Two-pass high-resolution sampling: a BASE pass from noise at the size the UNets were trained for, then a
    REFINE pass at a larger size that starts from the base result up-sampled (the panorama periodic in longitude), re-noised to
    the timestep ``strength`` selects, and runs only the tail of its schedule.  It owns two DenoiseLoops on the one model;
    ``run()`` is base.run(), refine.restart(init=SourceLatents(*base.result(), resample=...)), refine.run().  base.result() is in
    the caller's un-rotated frame, which is the frame SourceLatents is defined in: the rotation the base pass accumulated never
    reaches the refine pass.

    base_noise / noise: (latents, pano_latent) NOISE pairs at the base and at the final size (DenoiseLoop's first two
    arguments); every final dimension is an integer multiple of the base one, views and panorama independently.  Views of the
    same size in both passes (20 x 64 x 64 at 512x1024 -> 1024x2048) are passed through without resampling.
    steps: the base grid; refine_steps: the refine grid (default: steps), of which int(refine_steps * strength) run;
    resample: "nearest", "bilinear" or "bicubic"; the other arguments (guidance_rescale among them) as DenoiseLoop
    takes them, for both passes.
    Known regions and layout conditioning are NOT taken here: compose two DenoiseLoops by hand for them, the second with
    init=SourceLatents(..., resample=)."""

    def __init__(self, model, base_noise, noise, prompt_embd, pano_prompt_embd, cameras, *, steps=50, refine_steps=None,
                 strength=0.5, resample="bicubic", sampler="ddim", guidance_scale=9.0, rot_diff=90.0, use_graphs=False,
                 guidance_rescale=0.0):
        refine_steps = steps if refine_steps is None else refine_steps
        self._check_strength(refine_steps, strength)
        self.resample = resample
        # the refine loop's source buffers, at the size base.result() will have: checks the sizes against each other too
        placeholder = SourceLatents(torch.zeros_like(base_noise[0]), torch.zeros_like(base_noise[1]), resample=resample)
        placeholder.check(*noise)
        common = dict(rot_diff=rot_diff, guidance_scale=guidance_scale, use_graphs=use_graphs, sampler=sampler,
                      guidance_rescale=guidance_rescale)
        self.base = DenoiseLoop(model, base_noise[0], base_noise[1], prompt_embd, pano_prompt_embd, cameras, steps=steps, **common)
        self.refine = DenoiseLoop(model, noise[0], noise[1], prompt_embd, pano_prompt_embd, cameras, steps=refine_steps,
                                  strength=strength, init=placeholder, **common)

    @staticmethod
    def _check_strength(refine_steps, strength):
        if executed_steps(refine_steps, strength)[0] == refine_steps:
            raise ValueError("HiResLoop: strength %r runs the whole refine grid of %d from noise and ignores the base pass; "
                             "it must be < 1" % (strength, refine_steps))

    def prepare(self):
        """Untimed set-up of both passes: geometry tables and (use_graphs) one captured graph per rotation offset and size."""
        self.base.prepare()
        self.refine.prepare()

    def run(self):
        z = self.base.run()
        self.refine.restart(init=SourceLatents(*z, resample=self.resample))
        return self.refine.run()

    def restart(self, base_noise=None, noise=None, strength=None):
        """Re-arm both loops in place for the next seed (DenoiseLoop.restart: same buffers, same graphs); None keeps the value."""
        base_noise, noise = base_noise or (None, None), noise or (None, None)
        if strength is not None:
            self._check_strength(self.refine.steps, strength)
        for loop, pair in ((self.base, base_noise), (self.refine, noise)):           # all checks before anything changes
            shapes = tuple((1,) + tuple(t.shape[1:]) for t in (loop.lat, loop.pano))
            _check_shapes("restart", [(n, t, s) for n, t, s in zip(("latents", "pano_latent"), pair, shapes) if t is not None],
                          shapes)
        self.base.restart(*base_noise)
        self.refine.restart(*noise, strength=strength)

    def result(self):
        return self.refine.result()


def add_noise(sched, x, noise, t):
    """``scheduler.add_noise`` (diffusers DDIMScheduler / DDPMScheduler): sqrt(abar_t) x + sqrt(1 - abar_t) noise, t (b,) per sample."""
    out = torch.empty_like(x, dtype=torch.float32)
    for i, ti in enumerate(t.tolist()):
        a = float(sched.alphas_cumprod[ti])
        ops.axpby(x[i], noise[i], a ** 0.5, (1 - a) ** 0.5, out=out[i])
    return out


def training_step(model, vae_encoder, images, pano, cameras, prompt_embd, pano_prompt_embd, latent_pad=8, sched=None,
                  draws=None, generator=None, pers_layout_cond=None, pano_layout_cond=None):
    """The body of ``PanFusion.training_step`` (PanFusion.py:64-98) on the HIP path: VAE-encode the views and the circularly
    padded panorama, draw the timestep and the panorama noise, project that noise into the views (``init_noise``), add
    noise, ONE denoiser call without CFG, MSE on both predictions.  Returns (loss, loss_pers, loss_pano); ``loss.backward()``
    then fills the gradients of ``model.trainable_tensors()`` (the model must have been built ``differentiable=True``).

    images (b, m, 3, H, W), pano (b, 1, 3, Hp, Wp) in [-1, 1] on the GPU; cameras: dict of (b, m); the prompt embeddings as
    ``embed_prompt`` leaves them (b, m, L, D) / (b, 1, L, D) (text_encoder.TextEncoder).  draws: optional dict with the
    random draws (``eps_views``, ``eps_pano`` for the VAE posterior, ``t`` (b,), ``pano_noise`` (b, 1, 4, h, w)) -- what the
    tests fix to compare against the oracle; anything missing is drawn here.
    pers_layout_cond / pano_layout_cond: ``batch.get('images_layout_cond')`` / ``batch.get('pano_layout_cond')`` as the
    reference passes them (PanFusion.py:85-89).  Every ControlNet parameter that requires a gradient gets one (the
    reference's trainable set under layout_cond=True, PanoGenerator.py:153-157: all of them; train_engine.controlnet_backward);
    a ControlNet frozen with requires_grad_(False) contributes its residuals as constants."""
    from .utils.pano import pad_pano, unpad_pano
    from .vae import encode_image
    draws = draws or {}
    sched = sched or DDIMSchedule()
    dev = images.device
    latents = encode_image(images, vae_encoder, eps=draws.get("eps_views"), generator=generator)
    b, m, _, h, w = latents.shape
    pano_latent_pad = encode_image(pad_pano(pano, 8 * latent_pad), vae_encoder, eps=draws.get("eps_pano"), generator=generator)
    pano_latent = unpad_pano(pano_latent_pad, latent_pad).contiguous()
    t = draws.get("t")
    if t is None:
        t = torch.randint(0, sched.num_train_timesteps, (b,), device=dev, generator=generator)
    pano_noise = draws.get("pano_noise")
    if pano_noise is None:
        pano_noise = torch.randn(b, 1, 4, *pano_latent.shape[-2:], device=dev, generator=generator)
    pano_noise, noise = init_noise(pano_noise.to(dev).float(), cameras, h, w)
    noise_z = add_noise(sched, latents, noise, t)
    pano_noise_z = add_noise(sched, pano_latent, pano_noise, t)
    tt = t.to(dev).long()[:, None].repeat(1, m)
    denoise, pano_denoise = model(noise_z, pano_noise_z, tt, prompt_embd, pano_prompt_embd, cameras,
                                  pers_layout_cond, pano_layout_cond)
    loss_pers = torch.nn.functional.mse_loss(denoise, noise)
    loss_pano = torch.nn.functional.mse_loss(pano_denoise, pano_noise)
    return loss_pers + loss_pano, loss_pers, loss_pano
