"""The program of ONE rank of tests/test_gpu_sharded.py: the sharded denoiser on the real HIP kernels, every rank on cuda:0,
collectives over gloo.  Not collected by pytest; started as a fresh child process:

    python tests/sharded_worker.py --rank R --world N --port P --out DIR [--dtype fp16|bf16] [--precision mixed|fast]
                                   [--layout even] [--split a,b,...]

PF_SHARD_ATTN_MIN_TOKENS / PF_SHARD_ATTN_MIN_GROUP come from the environment (panfusion_amd.sharding reads them when it is
imported, which happens after the arguments are parsed).  Writes DIR/r<rank>.pt:
  views, cfg, has_pano, counts   this rank's place in the layout
  eps, pano_eps                  ONE denoiser call at t = 981 on this rank's CFG sample and views (pano_eps None off the owner)
  eager, graphed                 (latents, panorama) after 3 DDIM steps, launched eagerly / as hipGraph segments
  use_graphs, async, comm        loop.use_graphs after the graphed run, sharding.ASYNC, sharding.comm_stats(3) of the graphed run
"""
import argparse
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = 3
DTYPES = {"fp16": "float16", "bf16": "bfloat16"}


def build_model(dtype, precision=None):
    """The tiny dual-branch denoiser on the real ops (test_gpu_model.hip_model_from, with the precision scheme spelled out)."""
    from conftest import build_tiny_oracle
    from panfusion_amd.models.pano import MultiViewBaseModel
    om = build_tiny_oracle()
    m = MultiViewBaseModel(om.unet, om.pano_unet, None, None, om.pano_pad, compute_dtype=dtype, precision=precision)
    missing = m.load_state_dict({k: v for k, v in om.state_dict().items() if k.startswith("cp_blocks")}, strict=False)
    assert not [k for k in missing.missing_keys if k.startswith("cp_blocks")]
    return m


def tiny_inputs(dev):
    """mvgen_tiny.npz on `dev`: latents (2, 4, 4, 16, 16), panorama (2, 1, 4, 16, 32), prompts, and the cameras of ONE sample."""
    import torch
    from conftest import cam4, golden
    g = golden("mvgen_tiny.npz")
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    return t("latents"), t("pano_latent"), t("prompt_embd"), t("pano_prompt_embd"), {k: v[None] for k, v in cam4().items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp16")
    ap.add_argument("--precision", choices=("mixed", "fast"), default=None)
    ap.add_argument("--layout", default=None)
    ap.add_argument("--split", default=None)
    args = ap.parse_args(argv)
    split = tuple(int(v) for v in args.split.split(",")) if args.split else None

    import torch
    import torch.distributed as dist
    torch.set_num_threads(2)
    torch.cuda.set_device(0)
    dev = "cuda"
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % args.port, rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(minutes=2))
    try:
        from panfusion_amd import sharding
        model = build_model(getattr(torch, DTYPES[args.dtype]), args.precision)
        lat, pl, pe, ppe, cam1 = tiny_inputs(dev)
        shard = sharding.make_shard(4, layout=args.layout, split=split)
        res = dict(views=shard.views, cfg=shard.cfg, has_pano=shard.has_pano, counts=shard.counts)

        # 1. one denoiser call, driven as ShardedDenoiseLoop._local drives it
        model.shard = shard
        (v0, v1), c = shard.views, shard.cfg
        ts = torch.full((1, max(v1 - v0, 1)), 981, dtype=torch.long, device=dev)
        s, ps = model(lat[c:c + 1, v0:v1].contiguous(), pl[c:c + 1], ts, pe[c:c + 1, v0:v1], ppe[c:c + 1], cam1)
        torch.cuda.synchronize()
        res["eps"], res["pano_eps"] = s.cpu(), (ps.cpu() if ps is not None else None)

        # 2. / 3. the loop, eager and as hipGraph segments (prepare(): the untimed set-up that captures them, as bench.py runs it)
        def run_loop(graphs):
            loop = sharding.ShardedDenoiseLoop(model, shard, lat[:1], pl[:1], pe, ppe, cam1, steps=STEPS, use_graphs=graphs)
            if graphs:
                loop.prepare()
                sharding.reset_comm()
            out = [x.cpu() for x in loop.run()]
            torch.cuda.synchronize()
            return loop, out
        _, res["eager"] = run_loop(False)
        loop, res["graphed"] = run_loop(True)
        res["use_graphs"], res["async"], res["comm"] = bool(loop.use_graphs), bool(sharding.ASYNC), sharding.comm_stats(STEPS)
        torch.save(res, os.path.join(args.out, "r%d.pt" % args.rank))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
