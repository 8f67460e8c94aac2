"""The FAED auto-encoder's ENCODER on the HIP kernels (reference: models/faed/modules.py Encoder, CircularPadding, Conv2d, ResBlock,
ConvBlock): 17 convolutions, periodic in longitude and zero-padded in latitude, each one launch of ``pf_pano_conv`` with its bias and
evaluation-mode BatchNorm folded into the epilogue.

Inference only.  The reference's Decoder serves the auto-encoder's own training (FAED.training_step) and is not part of the metric:
it is out of scope here, and ``net.decoder.*`` tensors of a checkpoint are ignored."""
import math

import torch

from ... import ops

EPS = 1e-5          # nn.BatchNorm2d's default

# (module, ksize, stride, c_in, n_out, BatchNorm or None, relu, index of the layer whose output is added or None) in execution order
_LAYERS = []


def _conv(name, k, s, ci, co, norm=None, relu=False, res=None):
    _LAYERS.append((name + ".conv2d", k, s, ci, co, norm, relu, res))


def _conv_block(name, ci, co):                       # ConvBlock: conv, norm, ReLU
    _conv(name + ".conv1", 4, 2, ci, co, name + ".batchnorm1", True)


def _res_block(name, k, c):                          # ResBlock: conv, norm, ReLU, conv, norm, + input
    src = len(_LAYERS) - 1
    _conv(name + ".conv1", k, 1, c, c, name + ".batchnorm1", True)
    _conv(name + ".conv2", k, 1, c, c, name + ".batchnorm2", False, src)


_conv("downconv1_rgb", 9, 1, 3, 32)
_res_block("downres1_rgb", 9, 32)
_conv_block("downconv2_rgb", 32, 64)
_res_block("downres2_rgb", 7, 64)
_conv_block("downconv3_rgb", 64, 128)
_res_block("downres3_rgb", 5, 128)
_conv_block("downconv4_rgb", 128, 128)
_res_block("downres4_rgb", 3, 128)
_conv_block("downconv5_rgb", 128, 128)
_res_block("downres5_rgb", 3, 128)
_conv_block("downconv6_rgb", 128, 128)
_conv("fuse", 3, 1, 128, 128)
LAYERS = tuple(_LAYERS)
DOWNSAMPLE = 32                  # five stride-2 layers
OUT_CHANNELS = 128
PREFIX = "net.encoder."          # faed.ckpt holds the LightningModule's state_dict: FAED.net = AutoEncoder, .encoder = Encoder


def expected_keys():
    """name -> shape of every tensor of the reference Encoder's state_dict."""
    keys = {}
    for conv, k, s, ci, co, norm, relu, res in LAYERS:
        keys[conv + ".weight"] = (co, ci, k, k)
        keys[conv + ".bias"] = (co,)
        if norm:
            for part in ("weight", "bias", "running_mean", "running_var"):
                keys["%s.%s" % (norm, part)] = (co,)
            keys[norm + ".num_batches_tracked"] = ()
    return keys


def fold_batchnorm(bias, gamma=None, beta=None, mean=None, var=None, eps=EPS):
    """conv bias + evaluation-mode BatchNorm as one affine map of the bias-free sum, in float64:
    scale = gamma / sqrt(var + eps), shift = beta + (bias - mean) scale; (1, bias) without a norm."""
    bias = bias.double()
    if gamma is None:
        return torch.ones_like(bias), bias
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() + (bias - mean.double()) * scale


def flops_per_image(h, w):
    """Multiply-add FLOPs of the 17 convolutions on one h x w image."""
    total = 0
    for conv, k, s, ci, co, norm, relu, res in LAYERS:
        h, w = h // s, w // s
        total += 2 * h * w * co * k * k * ci
    return total


class Encoder:
    """``Encoder.from_state_dict(sd)(imgs)``: imgs [N, 3, H, W] uint8 or float on the 0..255 scale (H and W multiples of 32) ->
    the encoder's output [N, H/32, W/32, 128] float32, channels last.  ``features(imgs)`` is FAED.py get_activation: [N, 4 H] float32."""

    def __init__(self, layers, device, max_batch=4):
        self.layers = layers              # per layer (weight fp16 [n_out][k][k][c_in], scale fp32, shift fp32)
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.training = False
        self._acts = {}                   # (H, W) -> the 17 preallocated activations, for the largest chunk seen
        self._lat = {}

    @classmethod
    def from_state_dict(cls, sd, device="cuda", max_batch=4):
        """sd: the reference Encoder's tensors by name, bare or under ``net.encoder.`` (faed.ckpt's ``state_dict``; its decoder is not
        used).  Strict: a missing, unexpected or misshapen encoder tensor raises."""
        if any(k.startswith(PREFIX) for k in sd):
            sd = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
        want = expected_keys()
        missing, extra = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
        if missing or extra:
            raise KeyError("FAED encoder state_dict: missing %s, unexpected %s" % (missing, extra))
        sd = {k: torch.as_tensor(v) for k, v in sd.items()}
        for k, shape in want.items():
            if tuple(sd[k].shape) != shape:
                raise ValueError("FAED encoder state_dict: %s has shape %s, expected %s" % (k, tuple(sd[k].shape), shape))
        layers = []
        for conv, k, s, ci, co, norm, relu, res in LAYERS:
            bn = [sd["%s.%s" % (norm, p)] for p in ("weight", "bias", "running_mean", "running_var")] if norm else []
            scale, shift = fold_batchnorm(sd[conv + ".bias"], *bn)
            weight = sd[conv + ".weight"].permute(0, 2, 3, 1).contiguous()           # K ordered (ky, kx, c)
            layers.append((weight.to(device, torch.float16), scale.to(device, torch.float32).contiguous(),
                           shift.to(device, torch.float32).contiguous()))
        return cls(layers, device, max_batch)

    def train(self, mode=True):
        if mode:
            raise RuntimeError("the FAED encoder is inference only: BatchNorm is folded with its running statistics")
        return self

    def eval(self):
        return self

    def _activations(self, n, h, w):
        """The 17 activations for n <= max_batch images of h x w: views of one allocation per image size, which holds the largest chunk
        seen at that size (a batch's short last chunk reuses it), so scratch stays bounded by max_batch images."""
        imgs_h, imgs_w = h, w
        held = self._acts.get((h, w))
        if held is None or held[0].shape[0] < n:
            self._acts.clear()            # one image size at a time
            held = []
            for i, (conv, k, s, ci, co, norm, relu, res) in enumerate(LAYERS):
                h, w = h // s, w // s
                held.append(torch.empty(n, h, w, co, device=self.device, dtype=torch.float32 if i == len(LAYERS) - 1 else torch.float16))
            self._acts[(imgs_h, imgs_w)] = held
        return [a[:n] for a in held]

    def _run(self, imgs):
        n, _, h, w = imgs.shape
        acts = self._activations(n, h, w)
        x = imgs
        for i, ((conv, k, s, ci, co, norm, relu, res), (weight, scale, shift)) in enumerate(zip(LAYERS, self.layers)):
            x = ops.pano_conv(x, weight, scale, shift, k, s, relu=relu, residual=None if res is None else acts[res],
                              out_dtype=acts[i].dtype, out=acts[i])
        return x

    def _check(self, imgs):
        if self.training:
            raise RuntimeError("the FAED encoder is inference only")
        if imgs.dim() != 4 or imgs.shape[1] != 3:
            raise ValueError("FAED encoder: imgs must be [N, 3, H, W], got %s" % (tuple(imgs.shape),))
        if imgs.shape[2] % DOWNSAMPLE or imgs.shape[3] % DOWNSAMPLE:
            raise ValueError("FAED encoder: H and W must be multiples of %d, got %d x %d" % (DOWNSAMPLE, imgs.shape[2], imgs.shape[3]))
        imgs = imgs.to(self.device)
        return imgs if imgs.dtype in (torch.uint8, torch.float32) else imgs.float()

    def _chunks(self, imgs, fn):
        imgs = self._check(imgs)
        return torch.cat([fn(self._run(imgs[i:i + self.max_batch].contiguous())) for i in range(0, imgs.shape[0], self.max_batch)])

    @torch.no_grad()
    def __call__(self, imgs):
        return self._chunks(imgs, lambda x: x.clone())

    def latitude_weight(self, hp):
        """FAED.py:73-74, torch's own float32 values."""
        if hp not in self._lat:
            self._lat[hp] = torch.cos(torch.linspace(math.pi / 2, -math.pi / 2, hp, device=self.device))
        return self._lat[hp]

    @torch.no_grad()
    def features(self, imgs):
        return self._chunks(imgs, lambda x: ops.faed_features(x, self.latitude_weight(x.shape[1])))
