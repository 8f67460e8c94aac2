"""Times the FAED encoder (17 pf_pano_conv launches + pf_faed_features) per image at 512 x 1024, batch 4, on seeded weights, and the
same 17 layers composed from torch.nn.functional.pad(mode="circular") + conv2d in fp16 channels-last (what a user would run without
these kernels).  Device events around windows of whole passes (tens of milliseconds at least: --passes, and per layer as many
launches as fill --layer-ms), every shape warmed up, the versions alternated in one process (with --eight-rows also the encoder
with PF_PANO_CONV_ROWS=2, 8-row tiles everywhere); the achieved
FLOP rate is the convolutions' multiply-adds over the pass time, quoted against the 1.65-1.87 PFLOP/s that a pure-MFMA kernel
reaches under this chip's power cap (profiles/r6_gemm32_power_cap.txt).  Not part of bench.py.

    python tools/faed_bench.py [--batch 4] [--height 512] [--width 1024] [--repeats 5] [--passes 30] [--layers] [--layer-ms 50] [--eight-rows]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import faed_model as FM  # noqa: E402
from panfusion_amd import ops  # noqa: E402
from panfusion_amd.models.faed import modules as M  # noqa: E402

MFMA_UNDER_CAP = (1.65e15, 1.87e15)


class TorchComposition:
    """The same arithmetic from stock operators: fp16, channels-last, BatchNorm folded into the weights' scale and a bias."""

    def __init__(self, sd, device):
        self.layers = []
        for conv, k, s, ci, co, norm, relu, res in M.LAYERS:
            bn = [sd["%s.%s" % (norm, p)] for p in ("weight", "bias", "running_mean", "running_var")] if norm else []
            scale, shift = M.fold_batchnorm(sd[conv + ".bias"], *bn)
            w = (sd[conv + ".weight"].double() * scale[:, None, None, None]).to(device, torch.float16).contiguous(memory_format=torch.channels_last)
            self.layers.append((w, shift.to(device, torch.float16)))

    @torch.no_grad()
    def __call__(self, imgs):
        x = (imgs.float() / 127.5 - 1).half().contiguous(memory_format=torch.channels_last)
        outs = []
        for (conv, k, s, ci, co, norm, relu, res), (w, b) in zip(M.LAYERS, self.layers):
            p = 1 if s == 2 else (k - 1) // 2
            x = F.conv2d(F.pad(F.pad(x, (p, p, 0, 0), mode="circular"), (0, 0, p, p)), w, b, stride=s)
            if relu:
                x = F.relu_(x)
            if res is not None:
                x = x + outs[res]
            outs.append(x)
        m = x.float().mean(dim=3)
        weight = torch.cos(torch.linspace(np.pi / 2, -np.pi / 2, m.shape[-1], device=m.device))
        return (m * weight).reshape(m.shape[0], -1)


def timed(fn, passes):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(passes):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=30, help="encoder passes in one timed window (about 3 ms each at the defaults)")
    ap.add_argument("--layers", action="store_true", help="also time every layer alone")
    ap.add_argument("--layer-ms", type=float, default=50.0, help="length of a layer's timed window")
    ap.add_argument("--eight-rows", action="store_true", help="also time the encoder with 8-row tiles forced")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "faed_bench needs a GPU"
    dev = "cuda:0"
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in FM.state_dict(2024).items()}
    enc = M.Encoder.from_state_dict(sd, device=dev, max_batch=a.batch)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (a.batch, 3, a.height, a.width), generator=g, dtype=torch.uint8).to(dev)
    flops = M.flops_per_image(a.height, a.width)
    runs = {"pf_pano_conv": lambda: enc.features(imgs)}
    if a.eight_rows:
        def eight_rows():
            os.environ["PF_PANO_CONV_ROWS"] = "2"        # read by the library at every call
            try:
                return enc.features(imgs)
            finally:
                del os.environ["PF_PANO_CONV_ROWS"]
        assert "PF_PANO_CONV_ROWS" not in os.environ
        runs["pf_pano_conv_eight_row_tiles"] = eight_rows
    if not a.no_torch:
        comp = TorchComposition(sd, dev)
        runs["torch_composition"] = lambda: comp(imgs)
        f_hip, f_torch = runs["pf_pano_conv"]().double(), runs["torch_composition"]().double()
        print("features, kernels against the torch composition: rel-L2 %.2e" % float((f_hip - f_torch).norm() / f_torch.norm()))
    for fn in runs.values():                      # warm-up: code objects, algorithm choice, allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(a.repeats):                    # alternate the versions
        for name, fn in runs.items():
            times[name].append(timed(fn, a.passes))
    result = {"batch": a.batch, "height": a.height, "width": a.width, "gflop_per_image": flops / 1e9, "repeats": a.repeats, "passes": a.passes}
    for name, ts in times.items():
        med = float(np.median(ts))
        result[name] = {"ms_per_image_median": med / a.batch, "ms_per_image_min": min(ts) / a.batch, "ms_per_image_max": max(ts) / a.batch,
                        "tflops": flops * a.batch / (med * 1e-3) / 1e12,
                        "share_of_mfma_under_cap": [flops * a.batch / (med * 1e-3) / p for p in MFMA_UNDER_CAP[::-1]]}
    if a.layers:
        acts = enc._activations(a.batch, a.height, a.width)
        x, rows = imgs, []
        for i, ((conv, k, s, ci, co, norm, relu, res), (w, sc, sh)) in enumerate(zip(M.LAYERS, enc.layers)):
            run = lambda: ops.pano_conv(x, w, sc, sh, k, s, relu=relu, residual=None if res is None else acts[res], out_dtype=acts[i].dtype, out=acts[i])
            run()
            launches = max(5, min(20000, int(np.ceil(a.layer_ms / timed(run, 5)))))
            ms = float(np.median([timed(run, launches) for _ in range(a.repeats)]))
            fl = 2.0 * a.batch * acts[i].shape[1] * acts[i].shape[2] * co * k * k * ci
            rows.append({"layer": conv, "k": k, "stride": s, "c_in": ci, "n_out": co, "launches": launches, "ms": ms, "tflops": fl / (ms * 1e-3) / 1e12})
            x = acts[i]
        result["layers"] = rows
    print(json.dumps(result))


if __name__ == "__main__":
    main()
