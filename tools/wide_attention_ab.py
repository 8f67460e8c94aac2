"""A/B of the VAE mid-block attention core on one GPU: the flash kernel (ops.attention_wide) against the materialised form
(scores GEMM, row softmax, P V GEMM; query-chunked where one image's scores pass 2 GiB) on the same random q, k, V^T,
alternated inside one process.  Reports device time per form and run, 4 B N^2 D FLOP over it, and the transient bytes each
form allocates (peak above the operands).  profiles/wide_attention_ab.txt is this tool's output.

    python tools/wide_attention_ab.py [--runs 9] [--warmup 4] [--dtype fp16|bf16] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((20, 4096, 512), (1, 34816, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=4, help="untimed alternated runs per form before the timed ones")
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from panfusion_amd import ops
    from panfusion_amd import vae as PV
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[args.dtype]
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("wide attention A/B, %s, %d alternated runs per form after %d untimed ones (device events around each run; outputs pre-allocated; random normal q, k, v)" % (args.dtype, args.runs, args.warmup))
    for B, N, D in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * N)
        q, k = (torch.randn(B * N, D, device=dev, generator=g).to(dtype) for _ in range(2))
        vt = torch.randn(B, D, N, device=dev, generator=g).to(dtype)
        plan = PV.attention_plan(B, N, D, dtype, "materialised")

        out_f = torch.empty(B, N, D, device=dev, dtype=dtype)       # outputs allocated outside the timed region
        out_m = torch.empty(B * N, D, device=dev, dtype=dtype)

        def flash():
            return ops.attention_wide(q, k, vt, B, 1, D, N, N, q_ld=D, k_ld=D, vt_ld=N, q_bs=N * D, k_bs=N * D, vt_bs=D * N, out=out_f).view(B * N, D)

        def materialised(keep=False):
            # as in vae._attention: each pass's P V is consumed where it is (there by the output projection); `keep` copies the pieces
            # into one tensor for the agreement check only, outside the timed runs
            for rows, o in PV.materialised_attention(q, k, vt, B, N, D, dtype, plan):
                if keep:
                    out_m[rows] = o
            return out_m

        forms = (("flash", flash), ("materialised", materialised))
        ref = {}
        for name, f in forms:                                   # warm-up, agreement, transient memory
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ref[name] = f(True) if name == "materialised" else f()
            torch.cuda.synchronize()
            say("  B %2d N %5d D %d %-12s transient %.3f GB (outputs pre-allocated, not counted)" % (B, N, D, name, (torch.cuda.max_memory_allocated() - base) / 1e9))
        a, b = ref["flash"].double(), ref["materialised"].double()
        say("  B %2d N %5d D %d rel-L2 flash vs materialised %.3e (materialised: per %d, rows %d)" % (B, N, D, float((a - b).norm() / b.norm()), plan.per, plan.rows))
        del ref, a, b
        for _ in range(args.warmup):
            for name, f in forms:
                f()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        for _ in range(args.runs):
            for name, f in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        flop = 4.0 * B * N * N * D
        for name, _ in forms:
            t = sorted(times[name])
            say("  B %2d N %5d D %d %-12s ms %s   median %.3f ms = %.0f TF/s, min %.3f ms = %.0f TF/s"
                % (B, N, D, name, " ".join("%.3f" % x for x in times[name]), t[len(t) // 2], flop / t[len(t) // 2] / 1e9, t[0], flop / t[0] / 1e9))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
