"""The fixed grid of pf_conv_gemm problems behind tests/golden/gemm_plans.npz (tools/make_golden_gemm_plans.py writes it,
tests/test_gemm_plans.py reruns it): descriptors on fake, never dereferenced pointers, the three plan queries and the whole
pf_conv_plan of each, with and without GroupNorm moments, under the three settings of the knobs the planner reads per call.
Host arithmetic only: no GPU."""
import ctypes as C
import os

import numpy as np

from panfusion_amd import _lib

ENVS = ({}, {"PF_GEMM32": "1"}, {"PF_GN_EPILOGUE_RES": "1"})
LIVE_KNOBS = ("PF_GEMM32", "PF_GN_EPILOGUE_RES", "PF_CONV_FASTSEG")
PLAN_FIELDS = tuple(f for f, _ in _lib.ConvPlan._fields_)
COLUMNS = ("workspace_size", "gn_rows_query", "kernel_id") + tuple("p0_" + f for f in PLAN_FIELDS) + tuple("p1_" + f for f in PLAN_FIELDS)

# (n_img, h, w): M from 64 to 163 840 -- token rows of the linear layers, the UNet levels of the views and the panorama, VAE sizes
SHAPES = ((1, 1, 64), (2, 8, 16), (1, 16, 32), (8, 16, 32), (1, 32, 64), (1, 64, 128), (8, 32, 64), (4, 64, 128), (8, 64, 128),
          (20, 64, 128), (1, 1, 40960), (2, 1, 40960), (1, 1, 163840), (1, 128, 256))
C_IN = (64, 128, 320, 640, 1280, 2560)
N_OUT = (64, 128, 320, 512, 640, 1280, 2560)
CONVS = (dict(ksize=1), dict(ksize=3, pad=1), dict(ksize=3, pad=1, stride=2), dict(ksize=3, pad=1, upsample=1),
         dict(ksize=3, pad=1, upsample=1, subpixel=1), dict(ksize=3, pad=1, wrap_pad=2), dict(ksize=3, pad=1, crop=2),
         dict(ksize=3, pad=1, stride=2, wrap_pad=2, crop=1))
PLAIN = (dict(), dict(out_f32=True))
# operand mixes, on the 1x1 and the plain 3x3 problem (GEGLU: token layers only)
MIXES = (dict(rowvec=True), dict(res=16), dict(res=32, out_f32=True), dict(rowvec=True, res=16), dict(epilogue=2), dict(split3=1),
         dict(batch=4), dict(a1=True), dict(rowvec=True, out_f32=True))


def problems():
    """Every problem of the grid as a dict of options (the order is part of the fixture)."""
    out = []
    for n_img, h, w in SHAPES:
        for c0 in C_IN:
            for n_out in N_OUT:
                base = dict(n_img=n_img, h_in=h, w_in=w, c0=c0, n_out=n_out)
                for conv in CONVS:
                    for mix in PLAIN:
                        out.append(dict(base, **conv, **mix))
                for conv in CONVS[:2]:
                    for mix in MIXES:
                        out.append(dict(base, **conv, **mix))
                out.append(dict(base, ksize=1, epilogue=1))
    return out


def descriptor(n_img, h_in, w_in, c0, n_out, ksize=1, stride=1, pad=0, upsample=0, subpixel=0, wrap_pad=0, crop=0, out_f32=False,
               rowvec=False, res=0, epilogue=0, split3=0, batch=1, a1=False, dtype=_lib.PF_BF16):
    d = _lib.ConvDesc()
    d.a0, d.w, d.out, d.bias = 0x10000, 0x20000, 0x30000, 0x40000
    d.c0, d.a0_ld = c0, c0
    if a1:
        d.a1, d.c1, d.a1_ld = 0x50000, c0, c0
    d.n_img, d.h_in, d.w_in = n_img, h_in, w_in
    d.ksize, d.stride, d.pad, d.upsample, d.subpixel, d.wrap_pad, d.crop = ksize, stride, pad, upsample, subpixel, wrap_pad, crop
    d.h_out = ((h_in << upsample) + 2 * pad - ksize) // stride + 1
    d.w_out = (((w_in + 2 * wrap_pad) << upsample) + 2 * pad - ksize) // stride + 1 - 2 * crop
    d.n_out, d.epilogue, d.split3, d.batch = n_out, epilogue, split3, batch
    d.out_ld = n_out // 2 if epilogue == 1 else 2 * n_out if epilogue == 2 else n_out
    d.dtype = dtype
    d.out_dtype = _lib.PF_F32 if out_f32 else dtype
    d.res_dtype = dtype
    if rowvec:
        d.rowvec, d.rowvec_ld = 0x60000, n_out
    if res:
        d.residual, d.res_ld, d.res_dtype = 0x70000, n_out, (_lib.PF_F32 if res == 32 else dtype)
    if batch > 1:
        m = d.n_img * d.h_out * d.w_out
        d.a_bstride, d.w_bstride, d.out_bstride, d.res_bstride = m * c0, n_out * ksize * ksize * c0, m * d.out_ld, m * n_out
    return d


def plan(lib, d, want_moments):
    g = _lib.ConvPlan()
    assert lib.pf_conv_gemm_plan(C.byref(d), want_moments, C.byref(g)) == 0, lib.pf_last_error_string()
    return g


def row(lib, d):
    """One fixture row: COLUMNS of descriptor d."""
    r = [lib.pf_conv_gemm_workspace_size(C.byref(d)), lib.pf_conv_gemm_gn_rows(C.byref(d)), lib.pf_conv_gemm_kernel_id(C.byref(d))]
    for wm in (0, 1):
        g = plan(lib, d, wm)
        r += [getattr(g, f) for f in PLAN_FIELDS]
    return r


class live_env:
    """The planner's per-call knobs set to exactly `env` (the library reads them with getenv on every query)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in LIVE_KNOBS}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in LIVE_KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.saved.items() if v is not None})


def table(lib):
    """int64 [len(ENVS), len(problems()), len(COLUMNS)]"""
    descs = [descriptor(**p) for p in problems()]
    out = np.zeros((len(ENVS), len(descs), len(COLUMNS)), dtype=np.int64)
    for e, env in enumerate(ENVS):
        with live_env(env):
            for i, d in enumerate(descs):
                out[e, i] = row(lib, d)
    return out


def plan_class(p, g):
    """The plan class of pf_conv_plan fields g (a mapping) for problem options p: which launch arm of pf_conv_gemm runs it."""
    if p.get("subpixel"):
        return "subpixel_moments" if g["gn_rows"] else "subpixel"
    if g["kernel"] == 2:
        return "k32_tail" if g["m_split"] else "k32_moments" if g["gn_rows"] else "k32_whole_rounds"
    if g["kernel"] == 1:
        if g["m_split"]:
            return "8wave_tail_split"
        if g["splits"] > 1:
            return "8wave_split"
        return "8wave_%d%s" % (g["block_rows"], "_moments" if g["gn_rows"] else "")
    if g["ring_slots"] == 4:
        return "4wave_deep_ring_split" if g["splits"] > 1 else "4wave_deep_ring"
    if g["splits"] > 1:
        return "4wave_split"
    return "4wave_mrep%d%s" % (g["mrep"], "_moments" if g["gn_rows"] else "")


# (128-row tiles of the 4-wave kernel, mrep 4, need >= 512 of them -- at least 256 tiles of 256 rows, which the default knobs always give
# to the 8-wave kernel: only PF_GEMM8_MIN_TILES / PF_GEMM8_FILL settings reach that class, and those are read once per process)
CLASSES = ("4wave_mrep2", "4wave_mrep2_moments", "4wave_split", "4wave_deep_ring",
           "4wave_deep_ring_split", "8wave_256", "8wave_128", "8wave_256_moments", "8wave_128_moments", "8wave_split",
           "8wave_tail_split", "k32_whole_rounds", "k32_tail", "k32_moments", "subpixel", "subpixel_moments")


def smallest_members(tab):
    """class -> (MACs, env index, problem options, want_moments) of the smallest problem of the grid in that class."""
    probs, best = problems(), {}
    n = len(PLAN_FIELDS)
    ds = [descriptor(**p) for p in probs]
    all_macs = [d.n_img * d.h_out * d.w_out * d.n_out * d.ksize * d.ksize * (d.c0 + d.c1) * d.batch for d in ds]
    for e in range(len(ENVS)):
        for i, p in enumerate(probs):
            for wm in (0, 1):
                g = dict(zip(PLAN_FIELDS, tab[e, i, 3 + wm * n:3 + (wm + 1) * n]))
                macs, c = all_macs[i], plan_class(p, g)
                if c not in best or (macs, e) < best[c][:2]:
                    best[c] = (macs, e, p, wm)
    return best
