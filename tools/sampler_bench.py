"""DDIM vs DPM-Solver++(2M) on the benchmark configuration (cfg 2: 512x1024 panorama + 20 views of 512^2, CFG pair,
SD-2-base shapes, hipGraphs, bench.py's model and inputs).

    python tools/sampler_bench.py [--steps 20] [--repeats 2] [--out result.json]
    python tools/sampler_bench.py --profile          # short runs of both samplers, for rocprofv3 --kernel-trace --stats
    python tools/sampler_bench.py --known [--profile]  # DDIM without / with known content (inpainting)
    python tools/sampler_bench.py --strength 0.5       # DDIM at strength 1 / at strength S from a source
    python tools/sampler_bench.py --restart [--profile]  # set-up of another run: new loop + prepare() against restart()
    python tools/sampler_bench.py --hires [--profile]    # two-pass 512x1024 -> 1024x2048 (HiResLoop)
    python tools/sampler_bench.py --rescale [PHI] [--profile]  # DDIM without / with guidance rescale

Prints one JSON line:
  * ms_per_step -- the loop step (denoiser graph replay + the two update launches) of each sampler, timed after warm-up
    like bench.py, the samplers alternated ``--repeats`` times on the same model;
  * time_to_latents_s -- wall time from the first step to the final (un-rotated) latents of DDIM-50, 2M-25 and 2M-20
    (prepare(), i.e. tables and graph capture, untimed).
Fewer steps is what 2M is for; whether 2M-20/25 images match DDIM-50 in quality is NOT measured here (no trained weights).

With --known: ms_per_step of DDIM without and with a known region (a seeded panorama latent kept on half of the columns, its
nearest e2p in the views), alternated the same way; --profile then runs 6 steps of each.

With --rescale [PHI] (default 0.7): ms_per_step of DDIM without and with guidance_rescale = PHI -- two more launches per latent
and step, pf_cfg_moments and pf_cfg_rescaled_step_pair in place of pf_cfg_ddim_step_pair -- alternated the same way; --profile
then runs 6 steps of each.  Image quality with the rescale is NOT measured (no trained weights).

With --strength S: ms_per_step of DDIM at strength 1 and at strength S (a seeded source panorama latent and its nearest e2p in
the views; the grid is sized so that both run --warmup + --steps steps), alternated the same way, and time_to_latents_s of the
50-step grid at strength 1 and at strength S (int(50 S) steps).

With --restart: setup_ms -- wall time, to a synchronised device, of the two ways to set up another strength-S run (default 0.5)
on the 50-step grid: ``new_loop_prepare`` = DenoiseLoop(...) + prepare() (tables cached by the first loop, one graph capture
per rotation offset) and ``restart`` = DenoiseLoop.restart(new noise, new source) on a prepared loop; ``--repeats`` samples of
each, alternated.  pf_noised_start_pair is a latency-bound launch over 1.4 MB here, not tuned for bandwidth: its time is the
launch, see the kernel trace of --restart --profile (20 restarts, nothing else after the first prepare()).

With --hires: cfg 2 -> cfg 4 (the 64x128 panorama latent up-sampled to 128x256 under the same 20 views of 64x64 latents), graphs.
time_to_latents_s of HiResLoop.run() -- base pass, re-arming the refine loop from its result, refine pass -- with DDIM at
--base-steps 50 and with 2M at 20, strength --strength (default 0.5), and of a direct 50-step cfg 4 run from noise for
orientation; restart_ms -- wall time of HiResLoop.restart(new noise for both passes) to a synchronised device, ``--repeats``
samples.  --profile instead makes 20 launches each of upsampled_start_pair (bicubic, wrapped, the cfg 4 panorama latent) and of
the unfused pair it replaces, resize_latent + noised_start_pair, for rocprofv3 --kernel-trace --stats.  Image quality of the
two-pass result against the direct run is NOT measured (no trained weights).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed steps per ms_per_step sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dtype", default="fp16", choices=["bf16", "fp16"])
    ap.add_argument("--profile", action="store_true", help="6 steps of each sampler, no timing (run under rocprofv3)")
    ap.add_argument("--known", action="store_true", help="DDIM without / with known content instead of DDIM / 2M")
    ap.add_argument("--strength", type=float, default=None, help="DDIM at strength 1 / at this strength instead of DDIM / 2M")
    ap.add_argument("--restart", action="store_true", help="time DenoiseLoop + prepare() against restart() (set-up of another run)")
    ap.add_argument("--hires", action="store_true", help="two-pass cfg 2 -> cfg 4 through HiResLoop (DESIGN.md §4.8)")
    ap.add_argument("--base-steps", type=int, default=50, help="--hires: the DDIM grid of both passes (2M runs 20)")
    ap.add_argument("--rescale", type=float, nargs="?", const=0.7, default=None,
                    help="DDIM without / with guidance_rescale (default 0.7) instead of DDIM / 2M")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bench
    from panfusion_amd.models.sd2_unet_params import SD2_BASE
    from panfusion_amd.pipeline import DenoiseLoop, KnownRegion, SourceLatents, init_noise
    from panfusion_amd.utils.pano import icosahedron_sample_camera

    dev = torch.device("cuda", 0)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    cfg = dict(SD2_BASE)
    th, ph = icosahedron_sample_camera()
    model = bench.build_model(dev, dtype, cfg)
    inputs = bench.build_inputs(dev, 20, (64, 64), (64, 128), cfg["cross_attention_dim"], (np.degrees(th), np.degrees(ph)))

    known = None
    if args.known:
        g = torch.Generator().manual_seed(5)
        pano_z = torch.randn(inputs[1].shape, generator=g).to(dev)
        pano_m = torch.ones(1, 1, 1, *inputs[1].shape[-2:], device=dev)
        pano_m[..., :inputs[1].shape[-1] // 2] = 0.0
        cams, (h, w) = inputs[-1], inputs[0].shape[-2:]
        known = KnownRegion(init_noise(pano_z, cams, h, w)[1], init_noise(pano_m, cams, h, w)[1], pano_z, pano_m)

    def source(seed):
        pano_z = torch.randn(inputs[1].shape, generator=torch.Generator().manual_seed(seed)).to(dev)
        return SourceLatents(init_noise(pano_z, inputs[-1], *inputs[0].shape[-2:])[1], pano_z)

    def make(sampler, steps):
        kn, kw = None, {}
        if sampler == "ddim_known":
            sampler, kn = "ddim", known
        if sampler == "ddim_strength":
            # a grid on which strength S leaves exactly `steps` executed steps
            n = next(n for n in range(steps, 1001) if min(int(n * args.strength), n) == steps)
            sampler, steps, kw = "ddim", n, dict(strength=args.strength, init=source(5))
        if sampler == "ddim_rescale":
            sampler, kw = "ddim", dict(guidance_rescale=args.rescale)
        loop = DenoiseLoop(model, *inputs, steps=steps, use_graphs=True, sampler=sampler, known=kn, **kw)
        loop.prepare()
        return loop

    if args.hires:
        big = bench.build_inputs(dev, 20, (64, 64), (128, 256), cfg["cross_attention_dim"], (np.degrees(th), np.degrees(ph)))
        return hires_bench(args, torch, model, inputs, big)
    if args.restart:
        return restart_bench(args, torch, DenoiseLoop, model, inputs, source)

    samplers = ("ddim", "ddim_known") if args.known else ("ddim", "dpmpp_2m")
    if args.strength is not None:
        samplers = ("ddim", "ddim_strength")
    if args.rescale is not None:
        samplers = ("ddim", "ddim_rescale")
    if args.profile:
        for sampler in samplers:
            loop = make(sampler, 6)
            loop.run()
            torch.cuda.synchronize()
            del loop
        print(json.dumps({"profile": "%s, 6 steps each" % " and ".join(samplers)}))
        return

    per_step = {s: [] for s in samplers}
    for _ in range(args.repeats):
        for sampler in samplers:
            loop = make(sampler, args.steps + args.warmup)
            for _ in range(args.warmup):
                loop.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loop.step()
            torch.cuda.synchronize()
            per_step[sampler].append((time.perf_counter() - t0) / args.steps * 1e3)
            del loop
            torch.cuda.empty_cache()

    to_latents = {}
    runs = (("ddim_50", "ddim", 50), ("dpmpp_2m_25", "dpmpp_2m", 25), ("dpmpp_2m_20", "dpmpp_2m", 20))
    if args.strength is not None:
        runs = (("ddim_50", "ddim", 50), ("ddim_50_strength_%g" % args.strength, "ddim_strength", 50))
    for name, sampler, steps in (() if args.known or args.rescale is not None else runs):
        if sampler == "ddim_strength":
            loop = DenoiseLoop(model, *inputs, steps=steps, use_graphs=True, strength=args.strength, init=source(5))
            loop.prepare()
        else:
            loop = make(sampler, steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat, pano = loop.run()
        torch.cuda.synchronize()
        to_latents[name] = time.perf_counter() - t0
        assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(pano).all()), name
        del loop, lat, pano
        torch.cuda.empty_cache()

    res = {"workload": "cfg2: 512x1024 pano + 20x512^2 views, CFG pair, SD-2-base UNet shapes, hipGraphs, %s" % args.dtype,
           "ms_per_step": {k: [round(v, 3) for v in vs] for k, vs in per_step.items()},
           "time_to_latents_s": {k: round(v, 4) for k, v in to_latents.items()},
           "note": "image quality at 20 / 25 steps of 2M vs 50 of DDIM: not measured"}
    if args.strength is not None:
        res["note"] = "image quality at strength %g: not measured" % args.strength
    if args.rescale is not None:
        res["note"] = "image quality with guidance_rescale %g: not measured" % args.rescale
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def restart_bench(args, torch, DenoiseLoop, model, inputs, source):
    import json
    strength = 0.5 if args.strength is None else args.strength
    noise = lambda seed: torch.randn(inputs[1].shape, generator=torch.Generator().manual_seed(seed)).to(inputs[1].device)

    def fresh(seed):
        from panfusion_amd.pipeline import init_noise
        pano_n = noise(seed)
        lat_n = init_noise(pano_n, inputs[-1], *inputs[0].shape[-2:])[1]
        return lat_n, pano_n, source(seed + 100)

    loop = DenoiseLoop(model, *inputs, steps=50, use_graphs=True, strength=strength, init=source(5))
    loop.prepare()                                         # the first loop also builds the geometry tables: not a sample
    loop.run()
    torch.cuda.synchronize()
    if args.profile:
        for i in range(20):
            lat_n, pano_n, src = fresh(i)
            loop.restart(lat_n, pano_n, init=src)
        torch.cuda.synchronize()
        print(json.dumps({"profile": "20 restart() calls on a prepared cfg 2 loop"}))
        return
    setup = {"new_loop_prepare": [], "restart": []}
    for i in range(args.repeats):
        lat_n, pano_n, src = fresh(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        other = DenoiseLoop(model, lat_n, pano_n, *inputs[2:], steps=50, use_graphs=True, strength=strength, init=src)
        other.prepare()
        torch.cuda.synchronize()
        setup["new_loop_prepare"].append((time.perf_counter() - t0) * 1e3)
        want = other.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.restart(lat_n, pano_n, init=src)
        torch.cuda.synchronize()
        setup["restart"].append((time.perf_counter() - t0) * 1e3)
        got = loop.run()
        assert all(bool(torch.equal(a, b)) for a, b in zip(got, want)), "restart() and a fresh loop disagree"
        del other, want, got
        torch.cuda.empty_cache()
    res = {"workload": "cfg2: 512x1024 pano + 20x512^2 views, CFG pair, SD-2-base UNet shapes, hipGraphs, %s; 50-step grid at "
                       "strength %g" % (args.dtype, strength),
           "setup_ms": {k: [round(v, 3) for v in vs] for k, vs in setup.items()},
           "note": "restart() result checked bit for bit against the fresh loop of the same sample"}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def hires_bench(args, torch, model, inputs, big):
    import json
    from panfusion_amd import ops
    from panfusion_amd.pipeline import DenoiseLoop, HiResLoop, init_noise
    strength = 0.5 if args.strength is None else args.strength
    dev = inputs[1].device
    if args.profile:
        z = torch.randn(inputs[1].shape, generator=torch.Generator().manual_seed(5)).to(dev)
        n, out, out2, tmp = big[1], torch.empty_like(big[1]), torch.empty_like(big[1]), torch.empty_like(big[1])
        for _ in range(20):
            ops.upsampled_start_pair(z, n, 0.6, 0.8, 64, mode="bicubic", wrap=True, out=out, out2=out2)
        for _ in range(20):
            ops.noised_start_pair(ops.resize_latent(z, n.shape[-2:], "bicubic", True, out=tmp), n, 0.6, 0.8, 64, out=out, out2=out2)
        torch.cuda.synchronize()
        print(json.dumps({"profile": "20 x pf_upsampled_start_pair and 20 x (resize_latent + pf_noised_start_pair), 64x128 -> 128x256"}))
        return

    def noise(seed, like):
        pano_n = torch.randn(like[1].shape, generator=torch.Generator().manual_seed(seed)).to(dev)
        return init_noise(pano_n, inputs[-1], *like[0].shape[-2:])[1], pano_n

    to_latents, restart_ms = {}, []
    for name, sampler, steps in (("hires_ddim_%d" % args.base_steps, "ddim", args.base_steps), ("hires_dpmpp_2m_20", "dpmpp_2m", 20)):
        loop = HiResLoop(model, inputs[:2], big[:2], *inputs[2:], steps=steps, strength=strength, sampler=sampler, use_graphs=True)
        loop.prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat, pano = loop.run()
        torch.cuda.synchronize()
        to_latents[name] = time.perf_counter() - t0
        assert bool(torch.isfinite(lat).all()) and bool(torch.isfinite(pano).all()), name
        graphs = [dict(loop.base.graphs), dict(loop.refine.graphs)]
        for i in range(args.repeats if sampler == "ddim" else 0):
            base_n, n = noise(10 + i, inputs), noise(20 + i, big)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.restart(base_n, n)
            torch.cuda.synchronize()
            restart_ms.append((time.perf_counter() - t0) * 1e3)
        assert all(lp.graphs[k] is g[k] for lp, g in zip((loop.base, loop.refine), graphs) for k in g)
        del loop, lat, pano
        torch.cuda.empty_cache()
    direct = DenoiseLoop(model, *big, steps=50, use_graphs=True)
    direct.prepare()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    direct.run()
    torch.cuda.synchronize()
    to_latents["direct_cfg4_ddim_50"] = time.perf_counter() - t0
    res = {"workload": "cfg2 -> cfg4: 512x1024 -> 1024x2048 pano + 20x512^2 views, CFG pair, SD-2-base UNet shapes, hipGraphs, %s; "
                       "strength %g, bicubic" % (args.dtype, strength),
           "time_to_latents_s": {k: round(v, 4) for k, v in to_latents.items()},
           "restart_ms": [round(v, 3) for v in restart_ms],
           "note": "image quality of the two-pass result against the direct run: not measured"}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
