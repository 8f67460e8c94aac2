"""Float64 model of the FAED metric, written from its formulas (numpy only; no code of the reference).

The encoder is 17 convolutions, periodic in width and zero-padded in height:

  conv(x)[y][x][n] = bias[n] + sum_{ky,kx,c} x[y s - p + ky][(x s - p + kx) mod w][c] W[n][c][ky][kx]

followed, where the layer has one, by the evaluation-mode BatchNorm (v - mean) / sqrt(var + 1e-5) * gamma + beta, a ReLU, or the residual
sum of a ResBlock (conv-norm-ReLU, conv-norm, + input: no activation after the sum).  The feature vector of an image is the encoder's
output averaged over width, weighted by cos(latitude) of its row and flattened channel-major: f[c h' + y].  The distance between two
feature sets is |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum Re sqrt(eigvals(S1 S2)).

``conv_layer`` is one layer with the kernel's rounding points (fp16 operands, affine map, ReLU, residual), exact in float64, with the
magnitude sum that the tests' error bound needs."""
import numpy as np

EPS = 1e-5

# The 17 layers in execution order.  ``norm`` is the BatchNorm's key (None = none); ``res`` is the index of the layer whose OUTPUT is
# added after this one (a ResBlock's input).
LAYERS = []


def _add(name, k, s, ci, co, norm, relu, res=None):
    LAYERS.append(dict(name=name, conv=name + ".conv2d", k=k, s=s, ci=ci, co=co, norm=norm, relu=relu, res=res))


def _block(name, k, ci, co):
    _add(name + ".conv1", k, 2, ci, co, name + ".batchnorm1", True)


def _res(name, k, c):
    src = len(LAYERS) - 1                        # the layer before the block produces the block's input
    _add(name + ".conv1", k, 1, c, c, name + ".batchnorm1", True)
    _add(name + ".conv2", k, 1, c, c, name + ".batchnorm2", False, res=src)


_add("downconv1_rgb", 9, 1, 3, 32, None, False)
_res("downres1_rgb", 9, 32)
_block("downconv2_rgb", 4, 32, 64)
_res("downres2_rgb", 7, 64)
_block("downconv3_rgb", 4, 64, 128)
_res("downres3_rgb", 5, 128)
_block("downconv4_rgb", 4, 128, 128)
_res("downres4_rgb", 3, 128)
_block("downconv5_rgb", 4, 128, 128)
_res("downres5_rgb", 3, 128)
_block("downconv6_rgb", 4, 128, 128)
_add("fuse", 3, 1, 128, 128, None, False)
assert len(LAYERS) == 17


def pad_of(k, s):
    return 1 if s == 2 else (k - 1) // 2


def state_dict(seed):
    """All 109 tensors of the encoder by the names a checkpoint uses (without prefix), as numpy arrays: weights [n_out][c_in][k][k]
    ~ N(0, 1 / fan_in) (activations stay of order one through 17 layers), biases ~ N(0, 0.1), and a non-trivial BatchNorm."""
    rng = np.random.default_rng(seed)
    sd = {}
    for L in LAYERS:
        fan = L["ci"] * L["k"] * L["k"]
        out_gain = 0.05 if L["name"] == "fuse" else 1.0          # features of order 0.1, as a trained bottleneck's are
        sd[L["conv"] + ".weight"] = rng.normal(0.0, 1.0, (L["co"], L["ci"], L["k"], L["k"])) * (out_gain / np.sqrt(fan))
        sd[L["conv"] + ".bias"] = rng.normal(0.0, 0.1, L["co"]) * out_gain
        if L["norm"]:
            sd[L["norm"] + ".weight"] = rng.uniform(0.5, 1.5, L["co"])
            sd[L["norm"] + ".bias"] = rng.normal(0.0, 0.1, L["co"])
            sd[L["norm"] + ".running_mean"] = rng.normal(0.0, 0.2, L["co"])
            sd[L["norm"] + ".running_var"] = rng.uniform(0.5, 1.5, L["co"])
            sd[L["norm"] + ".num_batches_tracked"] = np.array(100, dtype=np.int64)
    assert len(sd) == 109
    return {k: (v if v.dtype == np.int64 else v.astype(np.float32)) for k, v in sd.items()}


def conv(x, w, k, s):
    """x [n][h][w][c] float64, w [n_out][k][k][c] float64 -> [n][h_out][w_out][n_out]: periodic columns, zero rows."""
    n, h, wd, c = x.shape
    p = pad_of(k, s)
    assert wd >= p
    cols = np.arange(-p, wd + p) % wd
    xp = np.zeros((n, h + 2 * p, wd + 2 * p, c))
    xp[:, p:p + h] = x[:, :, cols]
    ho, wo = (h + 2 * p - k) // s + 1, (wd + 2 * p - k) // s + 1
    out = np.zeros((n, ho, wo, w.shape[0]))
    for ky in range(k):
        for kx in range(k):
            out += xp[:, ky:ky + (ho - 1) * s + 1:s, kx:kx + (wo - 1) * s + 1:s] @ w[:, ky, kx].T
    return out


def fold(sd, L):
    """(scale, shift) float64 of a layer: v = conv_without_bias * scale + shift."""
    g = lambda key: np.asarray(sd[key], dtype=np.float64)
    bias = g(L["conv"] + ".bias")
    if not L["norm"]:
        return np.ones_like(bias), bias
    scale = g(L["norm"] + ".weight") / np.sqrt(g(L["norm"] + ".running_var") + EPS)
    return scale, g(L["norm"] + ".bias") + (bias - g(L["norm"] + ".running_mean")) * scale


def unfolded(sd, L, v):
    """The same map as written in the module: bias, then the norm."""
    g = lambda key: np.asarray(sd[key], dtype=np.float64)
    v = v + g(L["conv"] + ".bias")
    if L["norm"]:
        v = (v - g(L["norm"] + ".running_mean")) / np.sqrt(g(L["norm"] + ".running_var") + EPS) * g(L["norm"] + ".weight") + g(L["norm"] + ".bias")
    return v


def normalise(imgs):
    """[n][3][h][w] on the 0 .. 255 scale -> [n][h][w][3] float64 in [-1, 1]."""
    return np.transpose(np.asarray(imgs, dtype=np.float64), (0, 2, 3, 1)) / 127.5 - 1.0


def encoder(sd, imgs):
    """uint8 / float images [n][3][h][w] -> the encoder's output [n][h'][w'][128] in float64."""
    outs = []
    x = normalise(imgs)
    for L in LAYERS:
        w = np.transpose(np.asarray(sd[L["conv"] + ".weight"], dtype=np.float64), (0, 2, 3, 1))
        v = unfolded(sd, L, conv(x, w, L["k"], L["s"]))
        if L["relu"]:
            v = np.maximum(v, 0.0)
        if L["res"] is not None:
            v = v + outs[L["res"]]
        outs.append(v)
        x = v
    return x


def latitude_weight(hp):
    return np.cos(np.linspace(np.pi / 2, -np.pi / 2, hp))


def features_of(enc, weight=None):
    """[n][h'][w'][C] -> [n][C h']: mean over width, times the row weight, channel-major."""
    n, hp, wp, c = enc.shape
    weight = latitude_weight(hp) if weight is None else np.asarray(weight, dtype=np.float64)
    m = enc.mean(axis=2) * weight[None, :, None]            # [n][h'][C]
    return np.transpose(m, (0, 2, 1)).reshape(n, c * hp)


def features(sd, imgs):
    return features_of(encoder(sd, imgs))


def image_operand(imgs):
    """The image layer's fp16 operand: v / 127.5 - 1 in float32 (one division, one subtraction), rounded to fp16; [n][h][w][3]."""
    v = np.asarray(imgs).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
    return np.transpose(v, (0, 2, 3, 1)).astype(np.float16)


def conv_layer(x16, w16, k, s, scale, shift, relu=False, residual16=None):
    """One layer at the kernel's rounding points, in float64 on the given fp16 operands x16 [n][h][w][c], w16 [n_out][k][k][c] and
    fp32 scale / shift: -> (exact, mag) with exact = act(sum * scale + shift) (+ residual) and
    mag = sum |a w| |scale| + |shift| + |residual|, the magnitude the summation error is bounded by."""
    x, w = np.asarray(x16, dtype=np.float64), np.asarray(w16, dtype=np.float64)
    sc, sh = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    v = conv(x, w, k, s) * sc + sh
    mag = conv(np.abs(x), np.abs(w), k, s) * np.abs(sc) + np.abs(sh)
    if relu:
        v = np.maximum(v, 0.0)
    if residual16 is not None:
        r = np.asarray(residual16, dtype=np.float64).reshape(v.shape)
        v, mag = v + r, mag + np.abs(r)
    return v, mag


def perturb(imgs, seed):
    """A seeded perturbation of uint8 images (the 'generated' side of the metric tests): uniform noise of +-40 levels, clipped."""
    rng = np.random.default_rng(seed)
    return np.clip(imgs.astype(np.int64) + rng.integers(-40, 41, imgs.shape), 0, 255).astype(np.uint8)


def states(f):
    """The metric's three states of a feature set [n][d]: sum, f^T f, count."""
    f = np.asarray(f, dtype=np.float64)
    return f.sum(axis=0), f.T @ f, f.shape[0]


def frechet_from_states(s1, c1, n1, s2, c2, n2):
    if n1 < 2 or n2 < 2:
        raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
    m1, m2 = s1 / n1, s2 / n2
    cov1 = (c1 - n1 * np.outer(m1, m1)) / (n1 - 1)
    cov2 = (c2 - n2 * np.outer(m2, m2)) / (n2 - 1)
    ev = np.linalg.eigvals(cov1 @ cov2)
    return float(((m1 - m2) ** 2).sum() + np.trace(cov1) + np.trace(cov2) - 2.0 * np.sqrt(ev.astype(np.complex128)).real.sum())


def frechet(f1, f2):
    return frechet_from_states(*states(f1), *states(f2))
