"""Torch-tensor front end of the C-ABI HIP kernels.

PyTorch is used here for device memory and streams only: every function below
hands raw device pointers + sizes to ``libpanfusion_hip.so`` on the caller's
current stream.  No function has a torch / CPU fallback.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import (PF_BF16, PF_F16, PF_F32, PF_GN_FROM_PARTIALS, AttnBwdDesc, AttnBwdPlan, AttnDesc, AttnPlan, ConvDesc, ConvPlan, GnPlan,
                   LinearWsDesc, LwsPlan, check)

_DT = {torch.bfloat16: PF_BF16, torch.float16: PF_F16, torch.float32: PF_F32}

# When set to a list, every MFMA-kernel launch appends (kernel family, algorithmic FLOPs, start event,
# end event) -- used by bench.py's instrumented step for the roofline line.  None = no overhead.
TRACE = None


class _PlanCache(__import__("threading").local):
    """conv_gemm: problem shape -> [descriptor, plan without GroupNorm moments, plan with (asked on first use)] as the library plans it
    (pf_conv_gemm_plan).  The plans hold the live knobs PF_GEMM32 / PF_GN_EPILOGUE_RES as they were when asked: clear this cache after
    switching one (a moment launch on a stale plan is refused by the library: pf_conv_desc.gn_rows).  Per host
    THREAD (the cached descriptor's pointer members are rewritten on every call: two threads issuing the same shape must not
    share one) and bounded (variable batch sizes / resolutions: the oldest shape goes first)."""
    LIMIT = 4096

    def __init__(self):
        self.plans = {}


_PLANS = _PlanCache()
SPLITK_INKERNEL = os.environ.get("PF_SPLITK_INKERNEL") == "1"    # A/B switch, read once (as the library reads it)


def _traced(name, flops, launch, tag=""):
    if TRACE is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    TRACE.append((name, float(flops), e0, e1, tag))


def dt(t):
    return _DT[t.dtype if isinstance(t, torch.Tensor) else t]


try:                                     # raw handle of the current stream without building a torch.cuda.Stream object:
    _raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice      # 0.3 us against 8 us per
except AttributeError:                   # launch -- a third of the host time of a launch-bound step (tools/train_profile_host.py)
    _raw_stream = _cur_device = None


def _stream():
    if _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    """Row stride (elements) of a [.., rows, cols] tensor or column-sliced view of one."""
    assert t.stride(-1) == 1, "innermost dimension must be contiguous"
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


def _cams(fov, theta, phi):
    """Host double arrays (degrees) for the C ABI; accepts tensors / arrays / lists."""
    def host(v):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    f, t, p = host(fov), host(theta), host(phi)
    n = max(len(f), len(t), len(p))
    f, t, p = (np.ascontiguousarray(np.broadcast_to(a, (n,))) if len(a) != n else a for a in (f, t, p))
    as_p = lambda a: a.ctypes.data_as(_lib.c_dp)
    return n, (f, t, p), (as_p(f), as_p(t), as_p(p))


# ---------------------------------------------------------------------------- geometry
def e2p_grid(fov, theta, phi, eh, ew, h, w, device, want_lonlat=False):
    n, keep, (f, t, p) = _cams(fov, theta, phi)
    mx = torch.empty(n, h, w, device=device, dtype=torch.float32)
    my = torch.empty_like(mx)
    ll = torch.empty(n, h, w, 2, device=device, dtype=torch.float32) if want_lonlat else None
    check(_lib.lib().pf_e2p_grid(f, t, p, n, eh, ew, h, w, _p(mx), _p(my), _p(ll), _stream()), "pf_e2p_grid")
    return (mx, my, ll) if want_lonlat else (mx, my)


def p2e_grid(fov, theta, phi, ph, pw, h, w, device):
    n, keep, (f, t, p) = _cams(fov, theta, phi)
    mu = torch.empty(n, h, w, device=device, dtype=torch.float32)
    mv = torch.empty_like(mu)
    mask = torch.empty(n, h, w, device=device, dtype=torch.uint8)
    check(_lib.lib().pf_p2e_grid(f, t, p, n, ph, pw, h, w, _p(mu), _p(mv), _p(mask), _stream()), "pf_p2e_grid")
    return mu, mv, mask


def nearest_indices(map_x, map_y, src_h, src_w):
    idx = torch.empty(map_x.shape, device=map_x.device, dtype=torch.int32)
    check(_lib.lib().pf_nearest_indices(_p(map_x), _p(map_y), map_x.numel(), src_h, src_w, _p(idx), _stream()),
          "pf_nearest_indices")
    return idx


def remap(src, map_x, map_y, mode, mask=None):
    """src NCHW (fp32 / 16-bit), maps (B or 1, ho, wo) fp32."""
    src = src.contiguous()
    B, Cc, hs, ws = src.shape
    mb, ho, wo = map_x.shape
    out = torch.empty(B, Cc, ho, wo, device=src.device, dtype=src.dtype)
    check(_lib.lib().pf_remap(_p(src), dt(src), B, Cc, hs, ws, _p(map_x), _p(map_y), _p(mask), mb, ho, wo,
                              {"nearest": 0, "bilinear": 1}[mode], _p(out), _stream()), "pf_remap")
    return out


FEATHERS = {"horizontal": 0, "both": 1}


def mp2e(src, fov, theta, phi, out_hw, mode="bilinear", feather="horizontal", fill=255.0, want_weight=False):
    """src (B, m, C, ph, pw) (fp32 / 16-bit) -> the stitched panorama (B, C, H, W) fp32 (pf_mp2e), and the summed feather weight
    (B, 1, H, W) with ``want_weight``.  Cameras in degrees: B*m values each (per batch), or m shared by the whole batch."""
    if src.dim() != 5:
        raise ValueError("mp2e: src must be (B, m, C, ph, pw), got %s" % (tuple(src.shape),))
    if mode not in ("nearest", "bilinear") or feather not in FEATHERS:
        raise ValueError("mp2e: mode must be nearest or bilinear and feather one of %s, got %r, %r" % (sorted(FEATHERS), mode, feather))
    src = src.contiguous()
    B, m, Cc, ph, pw = src.shape
    n, keep, (f, t, p) = _cams(fov, theta, phi)
    if n != m and n != B * m:
        raise ValueError("mp2e: %d cameras for %d views (batch %d)" % (n, m, B))
    H, W = out_hw
    out = torch.empty(B, Cc, H, W, device=src.device, dtype=torch.float32)
    weight = torch.empty(B, 1, H, W, device=src.device, dtype=torch.float32) if want_weight else None
    nbytes = _lib.lib().pf_mp2e_workspace_size(B, m)
    ws = torch.empty(nbytes, device=src.device, dtype=torch.uint8)
    check(_lib.lib().pf_mp2e(_p(src), dt(src), B, m, Cc, ph, pw, f, t, p, B if n == B * m else 1, H, W,
                             {"nearest": 0, "bilinear": 1}[mode], FEATHERS[feather], float(fill), _p(out), _p(weight), _p(ws),
                             nbytes, _stream()), "pf_mp2e")
    return (out, weight) if want_weight else out


def equi_coords(H, W, device):
    out = torch.empty(H, W, 2, device=device, dtype=torch.float32)
    check(_lib.lib().pf_equi_coords(H, W, _p(out), _stream()), "pf_equi_coords")
    return out


def spherical_pe(coords, freq_bands):
    coords = coords.contiguous()
    n = coords.numel() // 2
    nf = freq_bands.numel()
    out = torch.empty(*coords.shape[:-1], 4 * nf, device=coords.device, dtype=torch.float32)
    check(_lib.lib().pf_spherical_pe(_p(coords), n, _p(freq_bands), nf, _p(out), _stream()), "pf_spherical_pe")
    return out


def epa_tables(fov, theta, phi, ph, pw, eh, ew, device):
    """-> bias_e [E, m*P], bias_p [m*P, E] (fp32, mask + 1), flags_e, flags_p (uint8 tile maps)."""
    m, keep, (f, t, p) = _cams(fov, theta, phi)
    E, P = eh * ew, ph * pw
    mP = m * P
    bias_e = torch.empty(E, mP, device=device, dtype=torch.float32)
    bias_p = torch.empty(mP, E, device=device, dtype=torch.float32)
    flags_e = torch.empty((E + 31) // 32, (mP + 31) // 32, device=device, dtype=torch.uint8)
    flags_p = torch.empty((mP + 31) // 32, (E + 31) // 32, device=device, dtype=torch.uint8)
    nbytes = _lib.lib().pf_epa_tables_workspace_size(m, ph, pw, eh, ew)
    ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
    check(_lib.lib().pf_epa_tables_build(f, t, p, m, ph, pw, eh, ew, _p(bias_e), _p(bias_p), _p(flags_e),
                                         _p(flags_p), _p(ws), nbytes, _stream()), "pf_epa_tables_build")
    return bias_e, bias_p, flags_e, flags_p


# ---------------------------------------------------------------------------- norms / pointwise
GN_FROM_EPILOGUE = os.environ.get("PF_GN_EPILOGUE", "1") != "0"      # A/B: 0 = always the separate statistics pass

# Arrival counters of the in-kernel split-K combine (pf_conv_desc.tickets): one zeroed int32 ring per device, handed out in
# slices of _TICKET_SLICE counters per split launch.  A slice is zero again when its launch has run (the last-arriving
# workgroup resets its counter) and comes round again only _TICKET_SLICES split launches later -- several denoiser steps --
# so no two launches that could overlap in time ever share one.  Allocated outside any graph capture (the warm-up pass).
_TICKET_SLICE, _TICKET_SLICES = 1024, 1024
_TICKETS = {}


def _ticket_slice(device):
    key = (device.type, device.index)
    ring = _TICKETS.get(key)
    if ring is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the split-K counter ring must be allocated before a graph capture (run one eager pass first)")
        ring = _TICKETS[key] = [torch.zeros(_TICKET_SLICE * _TICKET_SLICES, device=device, dtype=torch.int32), 0]
    off = ring[1]
    ring[1] = (off + 1) % _TICKET_SLICES
    return ring[0].data_ptr() + 4 * _TICKET_SLICE * off


def carry(dst, src):
    """dst = a view / reshape of src: hand over the GroupNorm moments a GEMM epilogue attached to src (`_pf_gn`)."""
    st = getattr(src, "_pf_gn", None)
    if st is not None:
        dst._pf_gn = st
    return dst


_GN_PLANS = _PlanCache()         # the arguments of pf_groupnorm_plan -> its GnPlan (nothing the plan reads changes inside a process)


def _gn_plan(key):
    """pf_groupnorm_plan of (n_img, hw, c0, c1, groups, dtype, rows0, rows1), asked once per problem; a refused problem raises."""
    plans = _GN_PLANS.plans
    g = plans.get(key)
    if g is None:
        g = GnPlan()
        check(_lib.lib().pf_groupnorm_plan(*key, C.byref(g)), "pf_groupnorm_plan")
        if len(plans) >= _GN_PLANS.LIMIT:
            plans.pop(next(iter(plans)))
        plans[key] = g
    return g


def groupnorm_scale_shift(x0, x1, n_img, hw, groups, eps, gamma, beta, ws=None, wrap=None):
    """x0 [n, hw, c0] (+ x1 [n, hw, c1] concatenated along channels) -> (scale, shift) [n, C] fp32.
    wrap = (image width, p): statistics of the tensor as if its width had been padded circularly by p columns (pad_pano).
    When every source still carries the per-column moments the GEMM that produced it left behind (conv_gemm(gn_stats=True)
    -> tensor attribute `_pf_gn` = (partials, rows per part)), the statistics come from those -- no pass over the tensors."""
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    Cc = c0 + c1
    scale = torch.empty(n_img, Cc, device=x0.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    st0 = getattr(x0, "_pf_gn", None)
    st1 = getattr(x1, "_pf_gn", None) if x1 is not None else None
    wrapped = wrap is not None and wrap[1] > 0
    offered = not wrapped and st0 is not None and (x1 is None or st1 is not None)
    # whether offered moments can serve is the library's decision (a linear layer's moment runs need not respect this consumer's
    # image boundaries, groups may hold odd numbers of channels): where they cannot, the plan is that of the statistics pass
    g = _gn_plan((n_img, hw, c0, c1, groups, dt(x0), st0[1] if offered else 0, st1[1] if offered and st1 else 0))
    if g.arm == PF_GN_FROM_PARTIALS:
        check(_lib.lib().pf_groupnorm_from_partials(_p(st0[0]), c0, st0[1], _p(st1[0]) if st1 else None, c1,
                                                    st1[1] if st1 else st0[1], n_img, hw, groups, eps, _p(gamma), _p(beta),
                                                    _p(scale), _p(shift), _stream()), "pf_groupnorm_from_partials")
        return scale, shift
    if wrapped or ws is None or ws.numel() < g.workspace_bytes:
        ws = torch.empty(g.workspace_bytes, device=x0.device, dtype=torch.uint8)
    if wrapped:
        check(_lib.lib().pf_groupnorm_stats_wrap(_p(x0), c0, _p(x1), c1, dt(x0), n_img, hw // wrap[0], wrap[0], wrap[1], groups, eps,
                                                 _p(gamma), _p(beta), _p(scale), _p(shift), _p(ws), ws.numel(), _stream()),
              "pf_groupnorm_stats_wrap")
    else:
        check(_lib.lib().pf_groupnorm_stats(_p(x0), c0, _p(x1), c1, dt(x0), n_img, hw, groups, eps, _p(gamma),
                                            _p(beta), _p(scale), _p(shift), _p(ws), ws.numel(), _stream()),
              "pf_groupnorm_stats")
    return scale, shift


def scale_shift_act(x0, x1, n_img, hw, scale, shift, act, out=None, out_dtype=None, split=False, raw_pair=False):
    """y = act(x * scale + shift) over the channel concat (x0 | x1); scale = shift = None: y = act(x).
    Sources 16-bit or fp32.  out_dtype: 16-bit type (default: the sources') or fp32; split=True: the
    16-bit pair [.., hi(C) | lo(C)] (A operand of a split-precision GEMM, engine.exact_gemm).
    raw_pair=True (fp32 sources, plain 16-bit y): also returns the UN-normalised input as that pair, written in the
    same pass -> (y, pair)."""
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    out_dtype = out_dtype or x0.dtype
    if out is None:
        out = torch.empty(n_img, hw, (c0 + c1) * (2 if split else 1), device=x0.device, dtype=out_dtype)
    else:
        _written(out)
    if raw_pair:
        assert x0.dtype == torch.float32 and not split and out_dtype != torch.float32
        pair = torch.empty(n_img, hw, 2 * (c0 + c1), device=x0.device, dtype=out_dtype)
        check(_lib.lib().pf_scale_shift_act_pair(_p(x0), c0, _p(x1), c1, n_img, hw, _p(scale), _p(shift), int(act),
                                                 dt(out_dtype), _p(out), _p(pair), _stream()), "pf_scale_shift_act_pair")
        return out, pair
    check(_lib.lib().pf_scale_shift_act(_p(x0), c0, _p(x1), c1, dt(x0), n_img, hw, _p(scale), _p(shift),
                                        int(act), dt(out_dtype), int(split), _p(out), _stream()), "pf_scale_shift_act")
    return out


def layernorm(x, gamma, beta, eps=1e-5, pe=None, out=None, out_dtype=None):
    """x [rows, C] 16-bit or fp32 -> 16-bit (out_dtype, default x.dtype); pe optional fp32 [pe_rows, C]
    (row r uses pe[r % pe_rows])."""
    rows, Cc = x.shape
    if out is None:
        out = torch.empty(rows, Cc, device=x.device, dtype=out_dtype or x.dtype)
    else:
        _written(out)
    check(_lib.lib().pf_layernorm(_p(x), _p(pe), 0 if pe is None else pe.shape[0], dt(x), rows, Cc,
                                  _p(gamma), _p(beta), eps, dt(out), _p(out), _stream()), "pf_layernorm")
    return out


def geglu(x, out=None):
    rows, two_inner = x.shape
    inner = two_inner // 2
    if out is None:
        out = torch.empty(rows, inner, device=x.device, dtype=x.dtype)
    else:
        _written(out)
    check(_lib.lib().pf_geglu(_p(x), dt(x), rows, inner, _p(out), _stream()), "pf_geglu")
    return out


def timestep_features(t, dim, dtype):
    """t: 1-D int64 (any stride: `timestep[:, 0]` of a (b, m) tensor is read in place)."""
    if t.dtype != torch.int64 or t.dim() != 1:
        t = t.to(torch.int64).reshape(-1).contiguous()
    out = torch.empty(t.numel(), dim, device=t.device, dtype=dtype)
    check(_lib.lib().pf_timestep_features_strided(_p(t), t.stride(0) if t.numel() > 1 else 1, t.numel(), dim, dt(dtype), _p(out), _stream()),
          "pf_timestep_features")
    return out


def _written(out):
    """An op wrote into a caller's `out=` buffer: GroupNorm moments it carried (`_pf_gn`, attached by a GEMM epilogue) described
    its previous contents."""
    if hasattr(out, "_pf_gn"):
        del out._pf_gn
    return out


def silu(x, out=None):
    if out is None:
        out = torch.empty_like(x)
    else:
        _written(out)
    check(_lib.lib().pf_silu(_p(x), dt(x), x.numel(), _p(out), _stream()), "pf_silu")
    return out


def add(a, b, out=None):
    """a + b in a's dtype (b may have another one: fp32 stream + 16-bit ControlNet residual)."""
    if out is None:
        out = torch.empty_like(a)
    else:
        _written(out)
    check(_lib.lib().pf_add(_p(a), dt(a), _p(b), dt(b), a.numel(), _p(out), _stream()), "pf_add")
    return out


def pad_width(x, pad, out=None):
    """x NHWC [n, h, w, C] -> circularly padded [n, h, w + 2 pad, C]."""
    n, h, w, Cc = x.shape
    if out is None:
        out = torch.empty(n, h, w + 2 * pad, Cc, device=x.device, dtype=x.dtype)
    else:
        _written(out)
    check(_lib.lib().pf_pad_width(_p(x), dt(x), n, h, w, Cc, pad, _p(out), _stream()), "pf_pad_width")
    return out


def crop_width(x, crop, out=None):
    n, h, w, Cc = x.shape
    if out is None:
        out = torch.empty(n, h, w - 2 * crop, Cc, device=x.device, dtype=x.dtype)
    else:
        _written(out)
    check(_lib.lib().pf_crop_width(_p(x), dt(x), n, h, w, Cc, crop, _p(out), _stream()), "pf_crop_width")
    return out


def pad_width_rows(x, pad):
    """Circular pad of the last axis of a contiguous tensor of any rank (pad_pano on NCHW)."""
    x = x.contiguous()
    w = x.shape[-1]
    rows = x.numel() // w
    out = torch.empty(*x.shape[:-1], w + 2 * pad, device=x.device, dtype=x.dtype)
    check(_lib.lib().pf_pad_width_rows(_p(x), x.element_size(), rows, w, pad, _p(out), _stream()),
          "pf_pad_width_rows")
    return out


def roll_width(x, shift, out=None):
    """torch.roll(x, shift, dims=-1) on a contiguous tensor."""
    x = x.contiguous()
    w = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    else:
        _written(out)
    check(_lib.lib().pf_roll_width_rows(_p(x), x.element_size(), x.numel() // w, w, int(shift), _p(out), _stream()),
          "pf_roll_width_rows")
    return out


def nchw_to_nhwc(x, dtype, out=None):
    x = x.contiguous()
    n, Cc, h, w = x.shape
    if out is None:
        out = torch.empty(n, h, w, Cc, device=x.device, dtype=dtype)
    else:
        _written(out)
    check(_lib.lib().pf_nchw_to_nhwc(_p(x), dt(x), n, Cc, h, w, dt(dtype), _p(out), _stream()), "pf_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, dtype, out=None):
    n, h, w, Cc = x.shape
    if out is None:
        out = torch.empty(n, Cc, h, w, device=x.device, dtype=dtype)
    else:
        _written(out)
    check(_lib.lib().pf_nhwc_to_nchw(_p(x), dt(x), n, Cc, h, w, dt(dtype), _p(out), _stream()), "pf_nhwc_to_nchw")
    return out


def embed_tokens(ids, tok, pos, Lp, out_dtype):
    """ids int64 [B, L]; tok [vocab, C], pos [>= L, C] fp32 -> [B, Lp, C] (rows >= L are zero)."""
    ids = ids.to(torch.int64).contiguous()
    B, L = ids.shape
    Cc = tok.shape[1]
    out = torch.empty(B, Lp, Cc, device=tok.device, dtype=out_dtype)
    check(_lib.lib().pf_embed_tokens(_p(ids), B, L, Lp, Cc, tok.shape[0], _p(tok), _p(pos), dt(out_dtype), _p(out), _stream()),
          "pf_embed_tokens")
    return out


def softmax_rows(scores, scale, out_dtype, out=None):
    """scores fp32 [..., rows, n] (contiguous rows) -> probabilities [..., rows, n] in out_dtype (16-bit)."""
    n = scores.shape[-1]
    rows = scores.numel() // n
    if out is None:
        out = torch.empty(scores.shape, device=scores.device, dtype=out_dtype)
    check(_lib.lib().pf_softmax_rows(_p(scores), rows, n, _ld(scores), float(scale), dt(out), _p(out), _ld(out), _stream()),
          "pf_softmax_rows")
    return out


def axpby(x, y, a, b, out=None):
    """a * x + b * y on fp32 tensors of one shape."""
    x, y = x.float().contiguous(), y.float().contiguous()
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().pf_axpby(_p(x), _p(y), float(a), float(b), x.numel(), _p(out), _stream()), "pf_axpby")
    return out


def vae_sample(moments, eps, scale):
    """moments fp32 NHWC [n, h, w, 2L] = (mean | logvar), eps fp32 NCHW [n, L, h, w] -> z fp32 NCHW
    = (mean + exp(0.5 clamp(logvar, -30, 20)) eps) * scale."""
    n, h, w, L2 = moments.shape
    z = torch.empty(n, L2 // 2, h, w, device=moments.device, dtype=torch.float32)
    check(_lib.lib().pf_vae_sample(_p(moments), _p(eps), n, L2 // 2, h * w, float(scale), _p(z), _stream()), "pf_vae_sample")
    return z


def tensor_to_image(x):
    """fp32 NCHW image in [-1, 1] -> uint8 NHWC (models/modules/utils.py:9-15)."""
    x = x.float().contiguous()
    n, Cc, h, w = x.shape
    out = torch.empty(n, h, w, Cc, device=x.device, dtype=torch.uint8)
    check(_lib.lib().pf_tensor_to_image(_p(x), n, Cc, h, w, _p(out), _stream()), "pf_tensor_to_image")
    return out


def cfg_ddim_step(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None):
    """x / eps fp32 [..., W]; coef = (sqrt a_t, sqrt(1-a_t), sqrt a_prev, sqrt(1-a_prev))."""
    W = x.shape[-1]
    rows = x.numel() // W
    if out is None:
        out = torch.empty_like(x)
    sa, sb, sap, sbp = (float(c) for c in coef)
    check(_lib.lib().pf_cfg_ddim_step(_p(x), _p(eps_uncond), _p(eps_cond), float(guidance), sa, sb, sap, sbp,
                                      rows, W, int(roll), _p(out), _stream()), "pf_cfg_ddim_step")
    return out


def _cfg_step_pair(entry, n_args, x, eps_uncond, eps_cond, guidance, coef, roll, out, out2, tstep, t_next, x0_prev=None, k=0.0,
                   x0_out=None, known=None, noise=None, mask=None, ka=0.0, kb=0.0, known_roll=0, partials=None, phi=0.0,
                   samples=1, factor_out=None):
    """The body of the four cfg_*_step_pair wrappers.  The C argument lists of their entry points are prefixes of one another
    with ``stream`` last: ``entry`` takes the first ``n_args`` of the one list built here.  Returns (out, x0_out)."""
    W = x.shape[-1]
    rows = x.numel() // W
    if out is None:
        out = torch.empty_like(x)
    assert x.is_contiguous() and out.is_contiguous() and (out2 is None or out2.is_contiguous())
    for t in (x0_out, x0_prev, known, noise, mask):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == x.numel())
    assert tstep is None or (tstep.dtype == torch.int64 and tstep.is_contiguous())
    n_partials = 0
    if partials is not None:
        assert partials.dtype == torch.float64 and partials.is_contiguous() and samples > 0
        assert partials.numel() % (samples * CFG_MOMENT_DOUBLES) == 0
        n_partials = partials.numel() // (samples * CFG_MOMENT_DOUBLES)
    assert factor_out is None or (factor_out.dtype == torch.float32 and factor_out.is_contiguous() and factor_out.numel() >= samples)
    sa, sb, sap, sbp = (float(c) for c in coef)
    # (a samples that does not divide rows reaches the entry point as a sample_rows that does not, and is refused there)
    sample_rows = rows // samples if rows % samples == 0 else rows + 1
    args = [_p(x), _p(eps_uncond), _p(eps_cond), float(guidance), sa, sb, sap, sbp, rows, W, int(roll), _p(out), _p(out2),
            _p(tstep), tstep.numel() if tstep is not None else 0, int(t_next),                      # ..16: pf_cfg_ddim_step_pair
            _p(x0_prev), float(k), _p(x0_out),                                                      # ..19: pf_cfg_dpmpp_step_pair
            _p(known), _p(noise), _p(mask), float(ka), float(kb), int(known_roll),                  # ..25: pf_cfg_inpaint_step_pair
            _p(partials), n_partials, sample_rows, float(phi), _p(factor_out)]                      # ..30: pf_cfg_rescaled_step_pair
    check(getattr(_lib.lib(), entry)(*args[:n_args], _stream()), entry)
    return out, x0_out


def cfg_ddim_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0):
    """cfg_ddim_step as the loop's one-launch state update: ``out`` may be ``x`` itself for any roll, ``out2`` receives a second
    copy (the other half of the CFG pair the next denoiser call reads), ``tstep`` (int64 device tensor) is set to ``t_next``."""
    return _cfg_step_pair("pf_cfg_ddim_step_pair", 16, x, eps_uncond, eps_cond, guidance, coef, roll, out, out2, tstep, t_next)[0]


def cfg_dpmpp_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                        x0_prev=None, k=0.0, x0_out=None):
    """cfg_ddim_step_pair with the DPM-Solver++(2M) correction: out = DDIM(x, eps) + k (x0 - x0_prev), and this step's x0 written
    to ``x0_out`` at the rolled position (the next step's history).  ``x0_prev=None``: a first-order step, out bit-identical to
    cfg_ddim_step_pair.  ``x0_out`` may be ``x0_prev`` itself; returns (out, x0_out)."""
    if x0_out is None:
        x0_out = torch.empty_like(x)
    return _cfg_step_pair("pf_cfg_dpmpp_step_pair", 19, x, eps_uncond, eps_cond, guidance, coef, roll, out, out2, tstep, t_next,
                          x0_prev, k, x0_out)


def cfg_inpaint_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                          x0_prev=None, k=0.0, x0_out=None, *, known, noise, mask, ka, kb, known_roll=0):
    """cfg_ddim_step_pair (``x0_out=None``) or cfg_dpmpp_step_pair (``x0_out`` given) followed by the known-region blend
    v <- m v + (1 - m) (ka known + kb noise) (mask 1 = generate, 0 = keep).  ``known`` / ``noise`` / ``mask``
    (fp32, the shape of x) are read at column (w - known_roll) mod W.  Returns (out, x0_out); x0_out is None in the DDIM form."""
    return _cfg_step_pair("pf_cfg_inpaint_step_pair", 25, x, eps_uncond, eps_cond, guidance, coef, roll, out, out2, tstep, t_next,
                          x0_prev, k, x0_out, known, noise, mask, ka, kb, known_roll)


CFG_MOMENT_DOUBLES = 4       # PF_CFG_MOMENT_DOUBLES: (sum c, sum c^2, sum e, sum e^2) per record
CFG_PARTIALS = 64            # records per sample the loop uses (a launch of 64 blocks per sample; any value in [1, 256] is valid)


def cfg_moments(eps_uncond, eps_cond, guidance, *, samples, out=None, n_partials=None):
    """First launch of guidance rescale: float64 partial sums of eps_cond and of the guided prediction
    fmaf(g, c - u, u), ``samples`` samples over the leading elements of the two fp32 tensors, ``n_partials`` records each, into
    ``out`` (float64, (samples, n_partials, 4); allocated when None -- a loop allocates it once and passes it every step).
    ``n_partials`` defaults to what ``out`` holds, to CFG_PARTIALS without one.  Deterministic: the same inputs give the same bits."""
    n = eps_cond.numel()
    assert eps_uncond.numel() == n and n % samples == 0
    for t in (eps_uncond, eps_cond):
        assert t.is_contiguous() and t.dtype == torch.float32
    if n_partials is None:
        n_partials = CFG_PARTIALS if out is None else out.numel() // (samples * CFG_MOMENT_DOUBLES)
    if out is None:
        out = torch.empty(samples, n_partials, CFG_MOMENT_DOUBLES, dtype=torch.float64, device=eps_cond.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == samples * n_partials * CFG_MOMENT_DOUBLES
    check(_lib.lib().pf_cfg_moments(_p(eps_uncond), _p(eps_cond), float(guidance), int(samples), n // samples, _p(out),
                                    int(n_partials), _stream()), "pf_cfg_moments")
    return out


def cfg_rescaled_step_pair(x, eps_uncond, eps_cond, guidance, coef, roll=0, out=None, out2=None, tstep=None, t_next=0,
                           x0_prev=None, k=0.0, x0_out=None, *, partials, phi, samples=1, factor_out=None,
                           known=None, noise=None, mask=None, ka=0.0, kb=0.0, known_roll=0):
    """cfg_inpaint_step_pair on the rescaled prediction eps = f eps_cfg, f = phi std(eps_cond) / std(eps_cfg) + 1 - phi per
    sample from ``partials`` (cfg_moments' output for the same predictions and guidance; x holds ``samples`` samples of equal
    size).  ``known`` / ``noise`` / ``mask`` all None: no blend (cfg_ddim_step_pair, or cfg_dpmpp_step_pair with ``x0_out``).
    ``factor_out`` (fp32, ``samples`` elements, or None) receives f.  Returns (out, x0_out)."""
    return _cfg_step_pair("pf_cfg_rescaled_step_pair", 30, x, eps_uncond, eps_cond, guidance, coef, roll, out, out2, tstep,
                          t_next, x0_prev, k, x0_out, known, noise, mask, ka, kb, known_roll, partials, phi, samples, factor_out)


def noised_start_pair(z, noise, ka, kb, roll=0, *, out, out2=None, tstep=None, t0=0):
    """The start state of a run in one launch: ``out`` <- ka z + kb noise rolled by ``roll`` along the width
    (``z=None``: the noise itself, a bit-exact rolled copy), ``out2`` a second copy (the CFG pair's other half), ``tstep`` (int64
    device tensor) set to ``t0``.  ``out`` / ``out2`` are existing buffers (captured graphs read them) and alias no input."""
    W = noise.shape[-1]
    rows = noise.numel() // W
    for t in (z, noise, out, out2):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == noise.numel())
    assert tstep is None or (tstep.dtype == torch.int64 and tstep.is_contiguous())
    opt = lambda t: _p(t) if t is not None else None
    check(_lib.lib().pf_noised_start_pair(opt(z), _p(noise), float(ka), float(kb), rows, W, int(roll), _p(out), opt(out2),
                                          opt(tstep), tstep.numel() if tstep is not None else 0, int(t0), _stream()),
          "pf_noised_start_pair")
    return out


RESIZE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}


def upsampled_start_pair(z, noise, ka, kb, roll=0, *, mode, wrap, out, out2=None, tstep=None, t0=0):
    """noised_start_pair with ``z`` (..., h, w) SMALLER than ``out`` (..., H, W) by integer factors: ``out`` <-
    ka r + kb noise rolled by ``roll``, r = torch's interpolate(z, (H, W), mode, align_corners=False) with clamped rows and --
    ``wrap=True`` -- periodic columns (a panorama latent; ``wrap=False`` clamps them: a view).  ``noise=None``: r itself, a pure
    resize.  ``mode``: "nearest", "bilinear" or "bicubic".  The leading dimensions of z and out must be equal."""
    if mode not in RESIZE_MODES:
        raise ValueError("resample mode must be one of %s, got %r" % (sorted(RESIZE_MODES), mode))
    (h, w), (H, W) = z.shape[-2:], out.shape[-2:]
    planes = z.numel() // (h * w)
    assert tuple(z.shape[:-2]) == tuple(out.shape[:-2]), (z.shape, out.shape)
    for t in (z, noise, out, out2):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
    for t in (noise, out2):
        assert t is None or t.numel() == out.numel()
    assert tstep is None or (tstep.dtype == torch.int64 and tstep.is_contiguous())
    opt = lambda t: _p(t) if t is not None else None
    check(_lib.lib().pf_upsampled_start_pair(_p(z), opt(noise), float(ka), float(kb), planes, h, w, H, W, RESIZE_MODES[mode],
                                             int(bool(wrap)), int(roll), _p(out), opt(out2), opt(tstep),
                                             tstep.numel() if tstep is not None else 0, int(t0), _stream()),
          "pf_upsampled_start_pair")
    return out


def resize_latent(x, size, mode="bicubic", wrap=False, out=None):
    """x fp32 (..., h, w) -> (..., *size), integer factors: upsampled_start_pair's resize alone (``noise=None``)."""
    if out is None:
        out = torch.empty(tuple(x.shape[:-2]) + tuple(size), device=x.device, dtype=torch.float32)
    assert tuple(out.shape[-2:]) == tuple(size)
    return upsampled_start_pair(x, None, 0.0, 0.0, 0, mode=mode, wrap=wrap, out=out)


# ---------------------------------------------------------------------------- GEMM / conv
def conv_gemm(a0, w, n_out, *, a1=None, n_img=1, h_in=1, w_in=None, ksize=1, stride=1, pad=0, upsample=0,
              bias=None, rowvec=None, residual=None, out=None, out_dtype=None, batch=1,
              a_bstride=0, w_bstride=0, out_bstride=0, res_bstride=0, a0_ld=None, a1_ld=None, c0=None, c1=None,
              out_ld=None, res_ld=None, geglu=False, algo_k=None, split_out=False, pad_hi=0, gn_stats=False,
              wrap_pad=0, crop=0, split3=False, plan_only=False, subpixel=False, a32_dtype=None, a_scale=None, a_shift=None,
              want_plan=False, split_k=True):
    """out[m, n] = sum_k A[m, k] W[n, k] (+bias +rowvec[img] +residual).  a0/a1 NHWC, the last
    dim is the channel stride; returns [M, n_out] (M = n_img * h_out * w_out).  The output takes the
    residual's dtype unless out_dtype says otherwise (fp32 residual stream in, fp32 out).
    algo_k: K of the layer for the FLOP count when the launched K carries split-precision passes.
    split_out: the result leaves as the 16-bit pair [M, 2 n_out] (per 32 columns [hi | lo]: operand of engine.exact_gemm).
    split3: a0 IS such a pair (c0 = 2 x channels) and w the matching [W_hi | W_lo] packing: three products per K block.
    pad_hi = 1: one more zero row / column at the bottom / right (F.pad(x, (0, 1, 0, 1)) of the VAE encoder's down-convs).
    gn_stats: the result feeds a GroupNorm -- where the kernel serving this problem can, its epilogue leaves the per-column
    moments of the output behind (attribute `_pf_gn` of the returned tensor, read by groupnorm_scale_shift).
    wrap_pad / crop: the input is read as if its width had been padded circularly by wrap_pad columns (pad_pano), the output
    loses `crop` columns on both sides (unpad_pano): pad -> conv -> crop of the panorama branch without the padded copies.
    subpixel: an upsampling convolution (ksize 3, upsample 1) as four 2x2 phase convolutions on the low-resolution grid; w = engine._subpixel_weight
    ([4 * n_out, 4 * C]): 4 instead of 9 MACs per output value and input channel (pf_conv_desc.subpixel).
    plan_only: launch nothing, return pf_conv_gemm_kernel_id of the problem (0 / 1: the 16x16x32 tile kernels, 2: the 32x32x16 kernel);
    want_plan: launch nothing, return the library's plan (ConvPlan) of the launch, with GroupNorm moments if gn_stats.
    split_k = False: no split-K scratch is handed over, so the library reduces K in ONE pass for every output tile (pf_conv_gemm plans without
    a split when pf_conv_desc.workspace is NULL): the launches of a host-side row split must not let the number of rows decide the
    summation order (vae.upsample_conv).
    a32_dtype (with split3, ksize 1): a0 / a1 are the fp32 tensors themselves (c0 / c1 fp32 channels) and a32_dtype the 16-bit type of the
    MFMA operands; the kernel forms the pair [hi | lo] of a0 | a1 (a_scale / a_shift [n_img, c0 + c1]: of their GroupNorm-applied values) while
    it stages them (pf_conv_desc.a_src_dtype) -- conv_gemm_a32 is the front end."""
    op_dtype = a32_dtype or a0.dtype                # type of the MFMA operands
    c0 = c0 if c0 is not None else a0.shape[-1]
    c1 = (c1 if c1 is not None else a1.shape[-1]) if a1 is not None else 0
    if w_in is None:
        w_in = a0.numel() // (a0.shape[-1] * max(batch, 1)) if ksize == 1 else None
    hl, wl = h_in << upsample, (w_in + 2 * wrap_pad) << upsample
    h_out = (hl + 2 * pad + pad_hi - ksize) // stride + 1
    w_out = (wl + 2 * pad + pad_hi - ksize) // stride + 1 - 2 * crop
    M = n_img * h_out * w_out
    if out is not None:
        out_dtype = out.dtype
    if split_out:
        out_dtype = op_dtype
    out_dtype = out_dtype or (residual.dtype if residual is not None else op_dtype)
    n_store = n_out // 2 if geglu else (2 * n_out if split_out else n_out)
    if out is None and not want_plan:                             # (a plan query allocates nothing)
        out = torch.empty((batch, M, n_store) if batch > 1 else (M, n_store), device=a0.device, dtype=out_dtype)
    a0_ld = a0_ld if a0_ld is not None else _ld(a0)
    a1_ld = (a1_ld if a1_ld is not None else _ld(a1)) if a1 is not None else 0
    rowvec_ld = _ld(rowvec) if rowvec is not None else 0
    res_ld = (res_ld if res_ld is not None else _ld(residual)) if residual is not None else 0
    res_dtype = dt(residual) if residual is not None else dt(op_dtype)
    out_ld = out_ld if out_ld is not None else (_ld(out) if out is not None else n_store)
    epilogue = 1 if geglu else (2 if split_out else 0)
    # One descriptor per problem SHAPE, filled once and reused (a launch-bound training step issues ~1500 of these per step:
    # the ~35 scalar members cost more host time than the call); with it the library's plans for the shape, asked once.  Per call
    # only the pointers change.
    pkey = (c0, c1, a0_ld, a1_ld, n_img, h_in, w_in, h_out, w_out, ksize, stride, pad, upsample, n_out, batch, epilogue, wrap_pad,
            crop, dt(op_dtype), dt(out_dtype), residual is not None, res_dtype, res_ld, rowvec is not None, rowvec_ld, bias is not None,
            out_ld, a_bstride, w_bstride, out_bstride, res_bstride, bool(split3), bool(subpixel), PF_F32 if a32_dtype else 0, a_scale is not None)
    plans = _PLANS.plans
    plan = plans.get(pkey)
    if plan is None:
        d = _conv_desc(pkey)
        d.a0, d.a1, d.w, d.bias, d.rowvec, d.residual, d.out = _p(a0), _p(a1), _p(w), _p(bias), _p(rowvec), _p(residual), _p(out)
        d.a_scale, d.a_shift = _p(a_scale), _p(a_shift)
        if len(plans) >= _PLANS.LIMIT:
            plans.pop(next(iter(plans)))
        plan = plans[pkey] = [d, _conv_plan(d, 0), None]
    d = plan[0]
    if plan_only:
        return plan[1].kernel
    d.a0, d.a1, d.w, d.bias, d.rowvec, d.residual, d.out = _p(a0), _p(a1), _p(w), _p(bias), _p(rowvec), _p(residual), _p(out)
    d.a_scale, d.a_shift = _p(a_scale), _p(a_shift)
    d.gn_partial, d.gn_rows, d.tickets, d.n_tickets = None, 0, None, 0
    if want_plan:
        if gn_stats and GN_FROM_EPILOGUE and batch == 1 and plan[2] is None:
            plan[2] = _conv_plan(d, 1)
        return plan[2] if gn_stats and GN_FROM_EPILOGUE and batch == 1 and plan[2].gn_rows > 0 else plan[1]
    g, gn = plan[1], None
    if gn_stats and GN_FROM_EPILOGUE and batch == 1:
        if plan[2] is None:
            plan[2] = _conv_plan(d, 1)
        if plan[2].gn_rows > 0:                # (else: a launch without moments, on the plan without)
            g = plan[2]
            gn = (torch.empty(M // g.gn_rows, 2, n_out // 2, device=a0.device, dtype=torch.float32), g.gn_rows)
            d.gn_partial, d.gn_rows = _p(gn[0]), g.gn_rows
    nbytes = g.workspace_bytes if split_k else 0
    ws = torch.empty(nbytes, device=a0.device, dtype=torch.uint8) if nbytes else None   # split-K slabs
    d.workspace, d.workspace_bytes = _p(ws), nbytes
    if nbytes and SPLITK_INKERNEL:
        # a split-K plan, combined inside the launch by the last-arriving workgroup (off by default: it does not pay at these
        # tile sizes, DESIGN.md 11.4 -- and without it no counter ring has to exist before a graph capture)
        d.tickets, d.n_tickets = _ticket_slice(a0.device), _TICKET_SLICE
    if TRACE is None:
        check(_lib.lib().pf_conv_gemm(C.byref(d), _stream()), "pf_conv_gemm")
    else:
        _traced("k_conv_gemm", 2.0 * M * n_out * (algo_k or ksize * ksize * (c0 + c1)) * batch,
                lambda: check(_lib.lib().pf_conv_gemm(C.byref(d), _stream()), "pf_conv_gemm"),
                "M%d N%d K%d k%d s%d u%d b%d%s" % (M, n_out, ksize * ksize * (c0 + c1) * (2 if a32_dtype else 1), ksize, stride, upsample, batch, " g32" if plan[1].kernel == 2 else " subpixel" if subpixel else ""))
    if gn is not None:
        out._pf_gn = gn                      # (a tensor that carries moments must not be written in place afterwards)
    elif hasattr(out, "_pf_gn"):
        del out._pf_gn                       # a reused out= buffer: moments of what it held before are stale now
    return out


def conv_gemm_a32(x0, w3, n_out, dtype, *, x1=None, scale=None, shift=None, n_img=1, w_in=None, **kw):
    """Split-precision 1x1 GEMM straight from the fp32 stream: x0 | x1 [.., C0] | [.., C1] fp32 (C0, C1 multiples of 32), optionally
    GroupNorm-applied (scale / shift [n_img, C0 + C1] of groupnorm_scale_shift; no activation), against w3 = engine._split_weight's
    [W_hi | W_lo] packing, MFMA operands of type dtype.  The result is bit for bit that of
    conv_gemm(scale_shift_act(x0, x1, .., split=True), w3, split3=True), without the pair tensor's round trip through memory: the
    kernels split every K block in registers while they stage it (same tile kernel, same plan, traced as that launch: K = 2 C)."""
    C0, C1 = x0.shape[-1], (x1.shape[-1] if x1 is not None else 0)
    if w_in is None:
        w_in = x0.numel() // (C0 * n_img)
    return conv_gemm(x0, w3, n_out, a1=x1, n_img=n_img, h_in=1, w_in=w_in, c0=C0, c1=C1 if x1 is not None else None,
                     algo_k=C0 + C1, split3=True, a32_dtype=dtype, a_scale=scale, a_shift=shift, **kw)


def conv_gemm_a32_serves(x0, w3, n_out, dtype, **kw):
    """Does conv_gemm_a32 serve this problem?  Everything but a GroupNorm-applied source (scale / shift) whose plan is the 256 x 160
    tile of the 8-wave kernel: its registers do not hold the affine operands (pf_conv_gemm refuses it); that problem keeps the pair form."""
    if kw.get("scale") is None:
        return True
    g = conv_gemm_a32(x0, w3, n_out, dtype, want_plan=True, **kw)     # (the plan cached with the shape's descriptor: nothing is allocated, nothing launched)
    return not (g.kernel == 1 and g.block_rows == 256 and g.nrep == 5)


def a32_ok(x0, x1=None):
    """Can conv_gemm_a32 take these sources?  fp32, channel counts that are multiples of 32, 16-byte aligned rows."""
    for t in (x0, x1):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.shape[-1] % 32 or t.stride(-1) != 1 or _ld(t) % 4 or t.data_ptr() % 16 or not t.is_contiguous():
            return False
    return True


def _conv_desc(pkey):
    """The scalar members of a pf_conv_desc from conv_gemm's problem key (the pointers are the caller's)."""
    d = ConvDesc()
    (d.c0, d.c1, d.a0_ld, d.a1_ld, d.n_img, d.h_in, d.w_in, d.h_out, d.w_out, d.ksize, d.stride, d.pad, d.upsample, d.n_out, d.batch,
     d.epilogue, d.wrap_pad, d.crop, d.dtype, d.out_dtype, _, d.res_dtype, d.res_ld, _, d.rowvec_ld, _, d.out_ld,
     d.a_bstride, d.w_bstride, d.out_bstride, d.res_bstride, d.split3, d.subpixel, d.a_src_dtype, _) = pkey
    return d


def _conv_plan(d, want_moments):
    """pf_conv_gemm_plan of a descriptor: the library's plan of the launch with / without GroupNorm moments."""
    g = ConvPlan()
    check(_lib.lib().pf_conv_gemm_plan(C.byref(d), want_moments, C.byref(g)), "pf_conv_gemm_plan")
    return g


def gemm_workspace_bytes(a0, w, n_out, *, a1=None, n_img=1, h_in=1, w_in=None, ksize=1, stride=1, pad=0,
                         upsample=0, batch=1, wrap_pad=0, crop=0, subpixel=False, **_):
    """Split-K scratch pf_conv_gemm wants for this problem (0: the K range is not split): room for the launch with and the
    launch without GroupNorm moments."""
    c0, c1 = a0.shape[-1], (a1.shape[-1] if a1 is not None else 0)
    if w_in is None:
        w_in = a0.numel() // (a0.shape[-1] * max(batch, 1))
    h_out = ((h_in << upsample) + 2 * pad - ksize) // stride + 1
    w_out = (((w_in + 2 * wrap_pad) << upsample) + 2 * pad - ksize) // stride + 1 - 2 * crop
    d = _conv_desc((c0, c1, c0, c1, n_img, h_in, w_in, h_out, w_out, ksize, stride, pad, upsample, n_out, batch, 0, wrap_pad, crop,
                    dt(a0), dt(a0), False, dt(a0), 0, False, 0, False, n_out, 0, 0, 0, 0, False, bool(subpixel), 0, False))
    d.a1 = _p(a1)
    return max(_conv_plan(d, 0).workspace_bytes, _conv_plan(d, 1).workspace_bytes)


# ---- weight-stationary linear (pf_linear_ws): the token layers of the three finest levels.  WHICH linear goes there is the library's
# decision (pf_linear_ws_plan, include/panfusion_hip.h -- shapes, thresholds and the PF_LINEAR_* knobs live there, read once per
# process): the front ends below map a call to a mode and ask.
LWS_16, LWS_F32, LWS_GEGLU, LWS_QKV, LWS_F32_LN, LWS_VT = 0, 1, 2, 3, 4, 5
_LWS_PLANS = _PlanCache()        # the scalar members of a pf_linear_ws_desc -> its LwsPlan (nothing the plan reads changes inside a process)


def _lws_key(x, w, mode, rows_per_batch=0):
    """The scalar members of the pf_linear_ws_desc of a call, (M, N, K, mode, a_ld, dtype, rows_per_batch) -- or None where the tensors
    themselves rule the kernel out: x not [rows, K] with unit inner stride, w not contiguous."""
    if x.dim() != 2 or x.stride(1) != 1 or not w.is_contiguous():
        return None
    return (x.shape[0], w.shape[0], x.shape[1], mode, x.stride(0), _DT.get(x.dtype, -1), rows_per_batch)


def _lws_desc(key):
    """A pf_linear_ws_desc with the scalar members of _lws_key (the pointers are the caller's)."""
    d = LinearWsDesc()
    d.M, d.N, d.K, d.mode, d.a_ld, d.dtype, d.rows_per_batch = key
    return d


def _lws_plan(key):
    """pf_linear_ws_plan of the problem _lws_key describes, asked once per problem."""
    plans = _LWS_PLANS.plans
    g = plans.get(key)
    if g is None:
        if len(plans) >= _LWS_PLANS.LIMIT:
            plans.pop(next(iter(plans)))
        g = plans[key] = LwsPlan()
        check(_lib.lib().pf_linear_ws_plan(C.byref(_lws_desc(key)), C.byref(g)), "pf_linear_ws_plan")
    return g


def _lws_preferred(x, w, mode, rows_per_batch=0):
    key = _lws_key(x, w, mode, rows_per_batch)
    return key is not None and _lws_plan(key).preferred != 0


def linear_ws_ok(rows, N, K, mode, x=None):
    """Do the front ends below send this problem to pf_linear_ws (x: the activations, for their dtype and row stride)?"""
    return _lws_plan((rows, N, K, mode) + ((K, PF_BF16) if x is None else (x.stride(-2) if x.stride(-1) == 1 else 0, _DT.get(x.dtype, -1))) + (0,)).preferred != 0


def linear_ws(x, w, mode, bias=None, residual=None, out=None, out_vt=None, rows_per_batch=0, ln=None, want_plan=False):
    """pf_linear_ws: x [rows, K] 16-bit, w [N, K] (the shapes at pf_linear_ws_desc, include/panfusion_hip.h).  mode LWS_16 -> [rows, N] 16-bit; LWS_F32 -> fp32 [rows, N] (+ fp32 residual);
    LWS_GEGLU -> [rows, N/2]; LWS_QKV (N = 960) -> ((q | k) [rows, 640], V^T [rows / rows_per_batch, 320, rows_per_batch]);
    LWS_F32_LN (N = 320, ln = (gamma, beta, eps)) -> (fp32 [rows, 320], LayerNorm of it in 16 bit [rows, 320]); LWS_VT
    -> the output transposed, [rows / rows_per_batch, N, rows_per_batch].
    want_plan: launch nothing, allocate nothing, return the library's plan (LwsPlan) of the launch."""
    key = _lws_key(x, w, mode, rows_per_batch)
    assert key is not None, "pf_linear_ws: x must be [rows, K] with a contiguous innermost dimension, w contiguous"
    if want_plan:
        return _lws_plan(key)
    rows, N, K = key[:3]
    d = _lws_desc(key)
    ln_out = None
    if mode == LWS_F32_LN:
        ln_out = torch.empty(rows, N, device=x.device, dtype=x.dtype)
        d.ln_gamma, d.ln_beta, d.ln_eps, d.ln_out, d.ln_ld = _p(ln[0]), _p(ln[1]), float(ln[2]), _p(ln_out), N
    if mode == LWS_QKV:
        nb = rows // rows_per_batch
        if out is None:
            out = torch.empty(rows, 640, device=x.device, dtype=x.dtype)
        if out_vt is None:
            out_vt = torch.empty(nb, 320, rows_per_batch, device=x.device, dtype=x.dtype)
        d.out_vt, d.vt_ld, d.vt_bs = _p(out_vt), out_vt.stride(1), out_vt.stride(0)
    elif mode == LWS_VT:
        nb = rows // rows_per_batch
        if out_vt is None:
            out_vt = torch.empty(nb, N, rows_per_batch, device=x.device, dtype=x.dtype)
        d.out_vt, d.vt_ld, d.vt_bs = _p(out_vt), out_vt.stride(1), out_vt.stride(0)
    elif out is None:
        out = torch.empty(rows, N // 2 if mode == LWS_GEGLU else N, device=x.device,
                          dtype=torch.float32 if mode in (LWS_F32, LWS_F32_LN) else x.dtype)
    d.a, d.w, d.bias = _p(x), _p(w), _p(bias)
    d.residual, d.res_ld = _p(residual), (_ld(residual) if residual is not None else 0)
    for buf in (out, out_vt):            # caller-supplied buffers: GroupNorm moments they carried described their OLD contents
        if buf is not None:
            _written(buf)
    d.out, d.out_ld = _p(out), (_ld(out) if out is not None else 0)
    if TRACE is None:
        check(_lib.lib().pf_linear_ws(C.byref(d), _stream()), "pf_linear_ws")
    else:
        _traced("k_linear_ws", 2.0 * rows * N * K, lambda: check(_lib.lib().pf_linear_ws(C.byref(d), _stream()), "pf_linear_ws"),
                "M%d N%d K%d mode%d" % (rows, N, K, mode))
    return (out, out_vt) if mode == LWS_QKV else (out, ln_out) if mode == LWS_F32_LN else out_vt if mode == LWS_VT else out


def linear_vt(x, w, n_batch):
    """The V projection of a self-attention written transposed, x [n_batch * nk, K] layer-normed tokens, w [N, K] -> V^T [n_batch, N, nk] (what
    pf_attention reads) -- on the weight-stationary kernel where the library prefers it for the shape, or None: the caller then takes the
    operand-swapped tile GEMM (linear_t)."""
    rows = x.shape[0]
    nk = rows // n_batch
    if nk * n_batch != rows or not _lws_preferred(x, w, LWS_VT, nk):
        return None
    return linear_ws(x, w, LWS_VT, rows_per_batch=nk)


def linear_ln(x, w, bias, residual, gamma, beta, eps):
    """out = x w^T + bias + residual (fp32 stream) together with LayerNorm(out) in 16 bit, in ONE launch where pf_linear_ws is preferred
    for the shape (C = 320: the row is complete inside a workgroup) -> (out, ln_out); (out, None) otherwise -- the caller then runs
    ops.layernorm itself."""
    if residual is not None and residual.dtype == torch.float32 and _lws_preferred(x, w, LWS_F32_LN):
        return linear_ws(x, w, LWS_F32_LN, bias=bias, residual=residual, ln=(gamma, beta, eps))
    return linear(x, w, bias=bias, residual=residual), None


def linear_qkv(x, wqkv, n_batch):
    """Self-attention projections in one launch: x [n_batch * nk, 320] layer-normed tokens, wqkv [960, 320] = (q | k | v)
    -> ((q | k) [rows, 640], V^T [n_batch, 320, nk]), or None where pf_linear_ws is not preferred for the shape."""
    nk = x.shape[0] // n_batch
    if not _lws_preferred(x, wqkv, LWS_QKV, nk):
        return None
    return linear_ws(x, wqkv, LWS_QKV, rows_per_batch=nk)


def linear(x, w, bias=None, residual=None, out=None, out_dtype=None, geglu=False, split_out=False, gn_stats=False):
    """x [rows, K] 16-bit, w [N, K] 16-bit.  geglu: w / bias rows interleaved (value_j, gate_j),
    returns [rows, N/2] = value * gelu(gate).  gn_stats: see conv_gemm (the moment runs are runs of token rows; the
    consumer's images must be whole runs, which groupnorm_scale_shift's entry point checks).
    The layers the library prefers on the weight-stationary kernel (pf_linear_ws_plan) go there."""
    rows, K = x.shape
    if not (split_out or gn_stats):
        odt = out.dtype if out is not None else (out_dtype or (residual.dtype if residual is not None else x.dtype))
        mode = None
        if geglu and residual is None and odt == x.dtype:
            mode = LWS_GEGLU
        elif not geglu and odt == torch.float32 and (residual is None or residual.dtype == torch.float32):
            mode = LWS_F32
        elif not geglu and residual is None and odt == x.dtype:
            mode = LWS_16
        if mode is not None and _lws_preferred(x, w, mode):
            return linear_ws(x, w, mode, bias=bias, residual=residual, out=out)
    return conv_gemm(x, w, w.shape[0], w_in=rows, bias=bias, residual=residual, out=out, out_dtype=out_dtype,
                     geglu=geglu, split_out=split_out, gn_stats=gn_stats)


def interleave_geglu(w, b=None):
    """[value rows | gate rows] (diffusers / reference GEGLU.proj, transformer.py:8-21) ->
    rows interleaved (value_0, gate_0, value_1, gate_1, ...) for the fused epilogue."""
    inner = w.shape[0] // 2
    wi = torch.stack([w[:inner], w[inner:]], 1).reshape(w.shape).contiguous()
    if b is None:
        return wi
    return wi, torch.stack([b[:inner], b[inner:]], 1).reshape(b.shape).contiguous()


def linear_t(x, w, out=None, ld=None):
    """Transposed projection for attention values: x [B, rows, K], w [N, K] ->
    out [B, N, ld] with out[b, n, r] = sum_k w[n,k] x[b,r,k]   (keys contiguous)."""
    B, rows, K = x.shape
    N = w.shape[0]
    ld = ld or ((rows + 31) // 32) * 32
    if out is None:
        out = torch.empty(B, N, ld, device=x.device, dtype=x.dtype)
    # roles swapped: GEMM rows = weight rows (N of them), GEMM columns = tokens
    conv_gemm(w, x, rows, w_in=N, out=out, out_ld=ld, batch=B,
              a_bstride=0, w_bstride=rows * K, out_bstride=N * ld, c0=K, a0_ld=K)
    return out


def conv_in(x, wgt, bias, cout, dtype, wrap=False, out=None):
    x = x.contiguous()
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty(n, h, w, cout, device=x.device, dtype=dtype)
    check(_lib.lib().pf_conv_in(_p(x), n, cin, h, w, _p(wgt), _p(bias), cout, int(wrap), dt(dtype), _p(out), _stream()),
          "pf_conv_in")
    return out


def conv_out(x, wgt, bias, cout, wrap=False, out=None):
    n, h, w, cin = x.shape
    if out is None:
        out = torch.empty(n, cout, h, w, device=x.device, dtype=torch.float32)
    check(_lib.lib().pf_conv_out(_p(x), dt(x), n, cin, h, w, _p(wgt), _p(bias), cout, int(wrap), _p(out), _stream()),
          "pf_conv_out")
    return out


def conv_out_weight_t(weight):
    """conv_out weight [cout <= 4, cin, 3, 3] -> fp32 [3, 3, cin, 4] (output channels padded with zeros): conv_out_gn's layout."""
    cout, cin = weight.shape[:2]
    wt = torch.zeros(3, 3, cin, 4, device=weight.device, dtype=torch.float32)
    wt[..., :cout] = weight.detach().float().permute(2, 3, 1, 0)
    return wt.contiguous()


def conv_out_gn(x, scale, shift, act, wgt_t, bias, cout, wrap=False, out=None):
    """conv_out(act(x * scale + shift)) in one launch: x fp32 [n, h, w, cin] before the GroupNorm, scale / shift [n, cin]."""
    n, h, w, cin = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and cin % 32 == 0 and cout <= 4
    if out is None:
        out = torch.empty(n, cout, h, w, device=x.device, dtype=torch.float32)
    check(_lib.lib().pf_conv_out_gn(_p(x), n, cin, h, w, _p(scale), _p(shift), int(act), _p(wgt_t), _p(bias), cout, int(wrap),
                                    _p(out), _stream()), "pf_conv_out_gn")
    return out


# ---------------------------------------------------------------------------- attention
def _attn_desc(q, k, vt, out, B, H, D, nq, nk, q_ld, k_ld, vt_ld, o_ld, q_bs, k_bs, vt_bs, o_bs, scale, bias=None, flags=None, lse=None):
    """pf_attn_desc of a launch, without scratch (attention adds it where the plan asks for some)."""
    d = AttnDesc()
    d.q, d.k, d.vt, d.out = _p(q), _p(k), _p(vt), _p(out)
    d.dtype, d.B, d.H, d.D, d.nq, d.nk = dt(q), B, H, D, nq, nk
    d.q_ld, d.k_ld, d.vt_ld, d.o_ld = q_ld, k_ld, vt_ld, o_ld
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = q_bs, k_bs, vt_bs, o_bs
    d.scale = scale if scale is not None else D ** -0.5
    d.bias, d.bias_ld = _p(bias), (_ld(bias) if bias is not None else 0)
    d.flags, d.flags_ld = _p(flags), (_ld(flags) if flags is not None else 0)
    d.lse = _p(lse)
    d.workspace, d.workspace_bytes = None, 0
    return d


def _attn_plan(d):
    g = AttnPlan()
    check(_lib.lib().pf_attention_plan(C.byref(d), C.byref(g)), "pf_attention_plan")
    return g


def attention(q, k, vt, B, H, D, nq, nk, *, q_ld, k_ld, vt_ld, o_ld=None, q_bs, k_bs, vt_bs, o_bs=None,
              scale=None, bias=None, flags=None, out=None, lse=None, want_plan=False):
    """lse: optional fp32 [B, H, nq] output (log2-domain log-sum-exp of the rows) for attention_bwd.
    want_plan: launch nothing, allocate nothing, return the library's plan (AttnPlan) of the launch."""
    o_ld = o_ld or H * D
    o_bs = o_bs if o_bs is not None else nq * o_ld
    if out is None and not want_plan:
        out = torch.empty(B, nq, o_ld, device=q.device, dtype=q.dtype)
    d = _attn_desc(q, k, vt, out, B, H, D, nq, nk, q_ld, k_ld, vt_ld, o_ld, q_bs, k_bs, vt_bs, o_bs, scale, bias, flags, lse)
    if want_plan:
        return _attn_plan(d)
    if bias is not None and lse is None:
        # few query blocks, many keys (the panorama-query direction of an EPA block): scratch that lets the library split the key range over more
        # workgroups (pf_attn_desc.workspace; a plan without scratch = this problem is not split)
        nbytes = _attn_plan(d).workspace_bytes
        if nbytes:
            ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
            d.workspace, d.workspace_bytes = _p(ws), nbytes
    _traced("k_attention", 4.0 * B * H * nq * nk * D,
            lambda: check(_lib.lib().pf_attention(C.byref(d), _stream()), "pf_attention"),
            "B%d H%d D%d nq%d nk%d bias%d" % (B, H, D, nq, nk, bias is not None))
    return out


WIDE_HEAD_DIMS = (128, 256, 512)


def attention_wide(q, k, vt, B, H, D, nq, nk, *, q_ld, k_ld, vt_ld, o_ld=None, q_bs, k_bs, vt_bs, o_bs=None, scale=None, out=None):
    """Flash attention at head widths 128 / 256 / 512 (pf_attention_wide): the operand layout of `attention`, no bias, no lse."""
    o_ld = o_ld or H * D
    o_bs = o_bs if o_bs is not None else nq * o_ld
    if out is None:
        out = torch.empty(B, nq, o_ld, device=q.device, dtype=q.dtype)
    d = _attn_desc(q, k, vt, out, B, H, D, nq, nk, q_ld, k_ld, vt_ld, o_ld, q_bs, k_bs, vt_bs, o_bs, scale)
    _traced("k_attention_wide", 4.0 * B * H * nq * nk * D,
            lambda: check(_lib.lib().pf_attention_wide(C.byref(d), _stream()), "pf_attention_wide"),
            "B%d H%d D%d nq%d nk%d" % (B, H, D, nq, nk))
    return out


# ---------------------------------------------------------------------------- training (EPA block backward)
def transpose_tokens(x, out=None):
    """x [B, T, C] (contiguous, 16-bit or fp32) -> [B, C, T]: the token-contiguous operand layout of the products whose
    reduction runs over tokens (attention backward, weight gradients)."""
    B, T, Cc = x.shape
    if out is None:
        out = torch.empty(B, Cc, T, device=x.device, dtype=x.dtype)
    if x.dtype == torch.float32:
        check(_lib.lib().pf_nhwc_to_nchw(_p(x), dt(x), B, Cc, 1, T, dt(out), _p(out), _stream()), "pf_nhwc_to_nchw")
    else:
        check(_lib.lib().pf_transpose_tokens(_p(x), dt(x), B, T, Cc, _p(out), _stream()), "pf_transpose_tokens")
    return out


def attention_delta(out, dout, B, H, D, nq):
    """rowsum(dout * out) per head: out / dout [B, nq, H*D] contiguous 16-bit -> fp32 [B, H, nq]."""
    delta = torch.empty(B, H, nq, device=out.device, dtype=torch.float32)
    check(_lib.lib().pf_attention_delta(_p(out), _p(dout), dt(out), B, H, D, nq, H * D, nq * H * D, _p(delta), _stream()),
          "pf_attention_delta")
    return delta


def _attn_bwd_desc(q, k, v, dout, qt, kt, dot, lse, delta, dq, dk, dv, B, H, D, nq, nk, q_ld, k_ld, v_ld, do_ld, dq_ld, dk_ld, dv_ld,
                   q_bs, k_bs, v_bs, do_bs, dq_bs, dk_bs, dv_bs, scale, bias, flags):
    """pf_attn_bwd_desc of a launch, without scratch (attention_bwd adds it where the plan asks for some)."""
    assert qt.dim() == 3 and kt.dim() == 3 and dot.dim() == 3 and qt.stride(-1) == kt.stride(-1) == dot.stride(-1) == 1
    d = AttnBwdDesc()
    d.q, d.k, d.v, d.dout = _p(q), _p(k), _p(v), _p(dout)
    d.qt, d.kt, d.dot = _p(qt), _p(kt), _p(dot)
    d.dq, d.dk, d.dv = _p(dq), _p(dk), _p(dv)
    d.dtype, d.B, d.H, d.D, d.nq, d.nk = dt(q), B, H, D, nq, nk
    d.q_ld, d.k_ld, d.v_ld, d.do_ld = q_ld, k_ld, v_ld, do_ld
    d.qt_ld, d.kt_ld, d.dot_ld = qt.stride(-2), kt.stride(-2), dot.stride(-2)      # (row slices of a wider transpose)
    d.dq_ld, d.dk_ld, d.dv_ld = dq_ld, dk_ld, dv_ld
    d.q_bs, d.k_bs, d.v_bs, d.do_bs = q_bs, k_bs, v_bs, do_bs
    d.qt_bs, d.kt_bs, d.dot_bs = qt.stride(0), kt.stride(0), dot.stride(0)
    d.dq_bs, d.dk_bs, d.dv_bs = dq_bs, dk_bs, dv_bs
    d.scale = scale if scale is not None else D ** -0.5
    if bias is not None:
        d.bias, d.bias_ld = _p(bias), _ld(bias)
    if flags is not None:
        d.flags, d.flags_ld = _p(flags), _ld(flags)
    d.lse, d.delta = _p(lse), _p(delta)
    return d                                                # (workspace NULL: a fresh struct is zero)


_BWD_PLAN = AttnBwdPlan()      # the launch path's plan, read at once (want_plan hands out a struct of its own)


def attention_bwd(q, k, v, dout, qt, kt, dot, lse, delta, dq, dk, dv, B, H, D, nq, nk, *, q_ld, k_ld, v_ld, do_ld,
                  dq_ld, dk_ld, dv_ld, q_bs, k_bs, v_bs, do_bs, dq_bs, dk_bs, dv_bs, scale=None, bias=None, flags=None, want_plan=False):
    """Backward of attention(): row-major q / k / v / dout (column views allowed: leading dimension + batch stride),
    transposed qt / kt / dot [B, H*D, tokens] (tokens contiguous; row slices of a wider transpose allowed),
    lse / delta fp32 [B, H, nq]; writes dq, dk, dv.
    want_plan: launch nothing, allocate nothing, return the library's plan (AttnBwdPlan) of the launch."""
    d = _attn_bwd_desc(q, k, v, dout, qt, kt, dot, lse, delta, dq, dk, dv, B, H, D, nq, nk, q_ld, k_ld, v_ld, do_ld, dq_ld, dk_ld, dv_ld,
                       q_bs, k_bs, v_bs, do_bs, dq_bs, dk_bs, dv_bs, scale, bias, flags)
    g = AttnBwdPlan() if want_plan else _BWD_PLAN
    lib, ref = _lib.lib(), C.byref(d)
    check(lib.pf_attention_bwd_plan(ref, C.byref(g)), "pf_attention_bwd_plan")
    if want_plan:
        return g
    nbytes = g.workspace_bytes
    if nbytes:                                              # few key blocks: scratch that lets the library split the query range (pf_attn_bwd_desc.workspace)
        ws = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = _p(ws), nbytes
    _traced("k_attention_bwd", 10.0 * B * H * nq * nk * D,
            lambda: check(lib.pf_attention_bwd(ref, _stream()), "pf_attention_bwd"),
            "B%d H%d D%d nq%d nk%d bias%d" % (B, H, D, nq, nk, bias is not None))


def colsum(x, out=None):
    """x [rows, N] (16-bit or fp32, rows may be strided) -> fp32 [N] column sums in a fixed order."""
    rows, N = x.shape
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    nbytes = _lib.lib().pf_colsum_workspace_size(rows, N)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    check(_lib.lib().pf_colsum(_p(x), dt(x), rows, N, _ld(x), _p(out), _p(ws), nbytes, _stream()), "pf_colsum")
    return out


def layernorm_bwd(x, gamma, dy, eps=1e-5, pe=None, dres=None, dx=None):
    """Backward of layernorm(x + pe): x [rows, C] (16-bit or fp32), dy fp32 [rows, C] (gradient of the normalised,
    affine output), dres optional fp32 gradient added to dx.  Returns (dx fp32, dgamma fp32 [C], dbeta fp32 [C])."""
    rows, Cc = x.shape
    if dx is None:
        dx = torch.empty(rows, Cc, device=x.device, dtype=torch.float32)
    parts = _lib.lib().pf_layernorm_bwd_parts(rows)
    partials = torch.empty(2, parts, Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().pf_layernorm_bwd(_p(x), _p(pe), 0 if pe is None else pe.shape[0], dt(x), rows, Cc, _p(gamma), eps,
                                      _p(dy), _p(dres), _p(dx), _p(partials), _stream()), "pf_layernorm_bwd")
    return dx, colsum(partials[0]), colsum(partials[1])


def geglu_bwd(u, dg, out=None):
    """u [rows, 2*inner] = [a | gate] (input of geglu), dg [rows, inner] -> du [rows, 2*inner]."""
    rows, two_inner = u.shape
    if out is None:
        out = torch.empty_like(u)
    check(_lib.lib().pf_geglu_bwd(_p(u), _p(dg), dt(u), rows, two_inner // 2, _p(out), _stream()), "pf_geglu_bwd")
    return out


def grad_scale_state(tensors):
    """Device-side power-of-two normalisation of a set of fp32 gradients (no host synchronisation): returns the
    4-float state tensor; state[1] = 2^-e with max|g| * 2^-e in [1, 2), state[2] = 2^e."""
    state = torch.empty(4, device=tensors[0].device, dtype=torch.float32)
    for i, t in enumerate(tensors):
        check(_lib.lib().pf_amax_f32(_p(t), t.numel(), _p(state), int(i == 0), _stream()), "pf_amax_f32")
    check(_lib.lib().pf_pow2_scale(_p(state), _stream()), "pf_pow2_scale")
    return state


def scale_by_state(x, state, index, out_dtype=torch.float32, out=None):
    """y = x * state[index] (x fp32 contiguous); out may alias x when fp32."""
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    else:
        _written(out)
    check(_lib.lib().pf_scale_f32(_p(x), x.numel(), _p(state), index, dt(out), _p(out), _stream()), "pf_scale_f32")
    return out


def groupnorm_bwd(x0, x1, n_img, hw, groups, eps, gamma, scale, shift, act, dy, dres=None):
    """Backward of scale_shift_act(groupnorm_scale_shift(..)): x0 [n, hw, c0] (+ x1 [n, hw, c1]), dy fp32 [n, hw, c0 + c1]
    -> (dx0, dx1) fp32 (dx1 None without a second source).  dres: fp32 gradient of the concat added to the result."""
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    dx0 = torch.empty(n_img, hw, c0, device=x0.device, dtype=torch.float32)
    dx1 = torch.empty(n_img, hw, c1, device=x0.device, dtype=torch.float32) if c1 else None
    nbytes = _lib.lib().pf_groupnorm_bwd_workspace_size(n_img, hw, groups)
    ws = torch.empty(nbytes, device=x0.device, dtype=torch.uint8)
    check(_lib.lib().pf_groupnorm_bwd(_p(x0), c0, _p(x1), c1, dt(x0), n_img, hw, groups, eps, _p(gamma), _p(scale), _p(shift),
                                      int(act), _p(dy), _p(dres), _p(dx0), _p(dx1), _p(ws), nbytes, _stream()), "pf_groupnorm_bwd")
    return dx0, dx1


def groupnorm_param_grads(x0, x1, n_img, hw, scale, shift, unit_scale, unit_shift, act, dy):
    """(dgamma, dbeta) fp32 [c0 + c1] of a trainable GroupNorm (+ SiLU) whose forward was scale_shift_act(x, scale, shift):
    unit_scale / unit_shift = groupnorm_scale_shift of the same input with gamma = 1, beta = 0 (xhat = x * unit_scale + unit_shift)."""
    c0 = x0.shape[-1]
    c1 = x1.shape[-1] if x1 is not None else 0
    Cc = c0 + c1
    out = torch.empty(2 * Cc, device=x0.device, dtype=torch.float32)
    nbytes = _lib.lib().pf_groupnorm_param_grads_workspace_size(n_img, hw, Cc)
    ws = torch.empty(nbytes, device=x0.device, dtype=torch.uint8)
    check(_lib.lib().pf_groupnorm_param_grads(_p(x0), c0, _p(x1), c1, dt(x0), n_img, hw, _p(scale), _p(shift), _p(unit_scale),
                                              _p(unit_shift), int(act), _p(dy), _p(out), _p(ws), nbytes, _stream()),
          "pf_groupnorm_param_grads")
    return out[:Cc], out[Cc:]


def silu_bwd(z, dy):
    """dy * silu'(z): z 16-bit or fp32 (any shape, contiguous), dy fp32 of the same shape -> fp32."""
    assert z.is_contiguous() and dy.is_contiguous() and dy.dtype == torch.float32 and z.shape == dy.shape
    out = torch.empty_like(dy)
    check(_lib.lib().pf_silu_bwd(_p(z), dt(z), _p(dy), z.numel(), _p(out), _stream()), "pf_silu_bwd")
    return out


def im2col3(x, stride=1):
    """x NHWC 16-bit [n, h, w, C] -> [n * ho * wo, 9 * C]: the nine zero-padded taps of a 3x3 / pad 1 convolution (tap-major,
    channels fastest: the column order of the packed conv weights [cout, ky, kx, cin])."""
    n, h, w, Cc = x.shape
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    out = torch.empty(n * ho * wo, 9 * Cc, device=x.device, dtype=x.dtype)
    check(_lib.lib().pf_im2col3(_p(x), dt(x), n, h, w, Cc, stride, _p(out), _stream()), "pf_im2col3")
    return out


def lora_fold(w, up, down, scale, out, out_t=None, d_out=None, u_out=None):
    """out [N, K] (16-bit, rows may be a slice of a packed weight) = w + scale * up @ down from fp32 w [N, K], up [N, r],
    down [r, K] (up = down = None: a plain conversion); optional by-products out_t [K, >= N] (transpose), d_out [r, >= K] (down)
    and u_out [r, >= N] (up^T) in the same 16-bit type, each a (possibly column-offset) view with contiguous rows."""
    N, K = w.shape
    r = 0 if up is None else up.shape[1]
    for t_ in (w, up, down):
        assert t_ is None or (t_.dtype == torch.float32 and t_.is_contiguous() and t_.device == out.device)
    for t_ in (out, out_t, d_out, u_out):
        assert t_ is None or (t_.stride(-1) == 1 and t_.dtype == out.dtype)
    ld = lambda t_: 0 if t_ is None else t_.stride(0)
    check(_lib.lib().pf_lora_fold(_p(w), _p(up), _p(down), N, K, r, float(scale), dt(out), _p(out), ld(out), _p(out_t), ld(out_t),
                                  _p(d_out), ld(d_out), _p(u_out), ld(u_out), _stream()), "pf_lora_fold")
    return out


def weighted_colsum(x, w, dev_scale=None, host_scale=1.0, blocks=None):
    """sum_t w[r, t] * x[t, c]: x [T, C] 16-bit (rows may be strided), w [R, T] fp32 (R a multiple of 4; rows go through the kernel in chunks of 16) -> fp32 [R, C]; with blocks
    = [(row0, rows, col0, cols), ...] (<= 4) a flat fp32 tensor holding only those blocks, each TRANSPOSED ([cols, rows]), one after
    the other.  dev_scale: optional 1-element fp32 device tensor multiplied into the result together with host_scale."""
    T, Cc = x.shape
    R = w.shape[0]
    assert w.dtype == torch.float32 and w.stride(1) == 1 and w.shape[1] >= T and x.stride(1) == 1
    if blocks:
        arr = (C.c_int * (4 * len(blocks)))(*[int(v) for b in blocks for v in b])
        out = torch.empty(sum(b[1] * b[3] for b in blocks), device=x.device, dtype=torch.float32)
    else:
        arr = None
        out = torch.empty(R, Cc, device=x.device, dtype=torch.float32)
    nbytes = _lib.lib().pf_weighted_colsum_workspace_size(T, Cc, R)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    check(_lib.lib().pf_weighted_colsum(_p(x), dt(x), T, Cc, x.stride(0), _p(w), R, w.stride(0), _p(dev_scale), float(host_scale),
                                        arr, len(blocks) if blocks else 0, _p(out), _p(ws), nbytes, _stream()), "pf_weighted_colsum")
    return out


def zero_insert2(x):
    """x NHWC 16-bit [n, h, w, C] -> [n, 2h, 2w, C] with x at the even positions (stride-2 conv data gradient)."""
    n, h, w, Cc = x.shape
    out = torch.empty(n, 2 * h, 2 * w, Cc, device=x.device, dtype=x.dtype)
    check(_lib.lib().pf_zero_insert2(_p(x), dt(x), n, h, w, Cc, _p(out), _stream()), "pf_zero_insert2")
    return out


def sum2x2(x):
    """x fp32 NHWC [n, 2h, 2w, C] -> [n, h, w, C] block sums (nearest x2 up-sampling backward)."""
    n, h2, w2, Cc = x.shape
    out = torch.empty(n, h2 // 2, w2 // 2, Cc, device=x.device, dtype=torch.float32)
    check(_lib.lib().pf_sum2x2(_p(x), n, h2 // 2, w2 // 2, Cc, _p(out), _stream()), "pf_sum2x2")
    return out


def pad_width_bwd(dy, pad):
    """Gradient of pad_width: dy fp32 [n, h, w + 2 pad, C] -> [n, h, w, C]."""
    n, h, wp, Cc = dy.shape
    out = torch.empty(n, h, wp - 2 * pad, Cc, device=dy.device, dtype=torch.float32)
    check(_lib.lib().pf_pad_width_bwd(_p(dy), n, h, wp - 2 * pad, Cc, pad, _p(out), _stream()), "pf_pad_width_bwd")
    return out


def crop_width_bwd(dy, crop):
    """Gradient of crop_width: dy fp32 [n, h, w - 2 crop, C] -> [n, h, w, C] (zero margins)."""
    n, h, wc, Cc = dy.shape
    out = torch.empty(n, h, wc + 2 * crop, Cc, device=dy.device, dtype=torch.float32)
    check(_lib.lib().pf_crop_width_bwd(_p(dy), n, h, wc + 2 * crop, Cc, crop, _p(out), _stream()), "pf_crop_width_bwd")
    return out


# ---------------------------------------------------------------------------- FAED encoder
_PANO_X = {torch.float16: PF_F16, torch.uint8: _lib.PF_U8, torch.float32: PF_F32}


def pano_conv(x, weight, scale, shift, ksize, stride, relu=False, residual=None, out_dtype=torch.float16, out=None):
    """One convolution of the FAED encoder (pf_pano_conv): periodic columns, zero rows, scale / shift epilogue, optional ReLU and residual.
    x is fp16 NHWC [n, h, w, c_in], or the image as delivered: uint8 / fp32 NCHW [n, 3, h, w] on the 0..255 scale (normalised while
    staged).  weight fp16 [n_out, k, k, c_in]; scale, shift fp32 [n_out]; residual fp16 [n, h_out, w_out, n_out].  -> [n, h_out, w_out, n_out]."""
    if x.dtype not in _PANO_X:
        raise ValueError("pano_conv: x must be float16 (NHWC) or uint8 / float32 (the NCHW image), got %s" % x.dtype)
    image = x.dtype != torch.float16
    x = x.contiguous()
    if image:
        n, c_in, h, w = x.shape
    else:
        n, h, w, c_in = x.shape
    n_out = weight.shape[0]
    if tuple(weight.shape) != (n_out, ksize, ksize, c_in) or weight.dtype != torch.float16 or not weight.is_contiguous():
        raise ValueError("pano_conv: weight must be contiguous float16 [n_out, %d, %d, %d], got %s %s" % (ksize, ksize, c_in, weight.dtype, tuple(weight.shape)))
    for name, v in (("scale", scale), ("shift", shift)):
        if v.dtype != torch.float32 or v.numel() != n_out or not v.is_contiguous():
            raise ValueError("pano_conv: %s must be contiguous float32 [%d]" % (name, n_out))
    pad = 1 if stride == 2 else (ksize - 1) // 2
    h_out, w_out = (h + 2 * pad - ksize) // max(stride, 1) + 1, (w + 2 * pad - ksize) // max(stride, 1) + 1
    if residual is not None and (residual.dtype != torch.float16 or residual.numel() != n * h_out * w_out * n_out or not residual.is_contiguous()):
        raise ValueError("pano_conv: residual must be contiguous float16 [%d, %d, %d, %d]" % (n, h_out, w_out, n_out))
    if out is None:
        out = torch.empty(n, max(h_out, 0), max(w_out, 0), n_out, device=x.device, dtype=out_dtype)
    elif out.dtype != out_dtype or out.numel() != n * h_out * w_out * n_out or not out.is_contiguous():
        raise ValueError("pano_conv: out must be contiguous %s [%d, %d, %d, %d]" % (out_dtype, n, h_out, w_out, n_out))
    d = _lib.PanoConvDesc()
    d.x, d.x_dtype, d.n_img, d.h, d.w, d.c_in = _p(x), _PANO_X[x.dtype], n, h, w, c_in
    d.weight, d.n_out, d.ksize, d.stride = _p(weight), n_out, ksize, stride
    d.scale, d.shift, d.relu, d.residual = _p(scale), _p(shift), int(bool(relu)), _p(residual)
    d.out, d.out_dtype = _p(out), _DT.get(out_dtype, -1)
    flops = 2.0 * n * h_out * w_out * n_out * ksize * ksize * c_in
    _traced("pano_conv", flops, lambda: check(_lib.lib().pf_pano_conv(C.byref(d), _stream()), "pf_pano_conv"))
    return out


def pano_conv_tile_rows(ksize, stride, n, h, w):
    """The output rows (8 or 16) of the tile a workgroup of pano_conv owns for n images of h x w (pf_pano_conv_tile_rows; no launch)."""
    rows = _lib.lib().pf_pano_conv_tile_rows(ksize, stride, n, h, w)
    if rows == 0:
        raise ValueError("pano_conv_tile_rows: pano_conv does not take ksize %d, stride %d on %d x %d x %d" % (ksize, stride, n, h, w))
    return rows


def faed_features(x, weight):
    """The encoder's output x fp32 [n, h', w', C] -> [n, C h'] fp32: mean over w', times weight[y], channel-major (pf_faed_features)."""
    if x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4 or weight.numel() != x.shape[1]:
        raise ValueError("faed_features: x must be float32 [n, h, w, C] and weight float32 [h]")
    x, weight = x.contiguous(), weight.contiguous()
    n, h, w, Cc = x.shape
    out = torch.empty(n, Cc * h, device=x.device, dtype=torch.float32)
    check(_lib.lib().pf_faed_features(_p(x), n, h, w, Cc, _p(weight), _p(out), _stream()), "pf_faed_features")
    return out
