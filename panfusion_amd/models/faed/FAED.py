"""Fréchet Auto-Encoder Distance (reference: models/faed/FAED.py FrechetAutoEncoderDistance, used by EvalPanoGen.test_step).

The reference class is a torchmetrics ``Metric``; this one has the same interface and states without that dependency: ``merge`` is
what ``dist_reduce_fx="sum"`` does across ranks, and ``compute`` writes out torchmetrics 1.3.2's ``_compute_fid``."""
import torch

from .modules import Encoder

_STATES = ("real_features_sum", "real_features_cov_sum", "real_features_num_samples",
           "fake_features_sum", "fake_features_cov_sum", "fake_features_num_samples")


class FrechetAutoEncoderDistance:
    higher_is_better = False

    def __init__(self, pano_height, encoder=None, device=None):
        """encoder: an ``Encoder`` (None: a metric that is only merged into / computed from given states)."""
        self.encoder = encoder
        device = torch.device(device if device is not None else (encoder.device if encoder is not None else "cpu"))
        self.num_features = num_features = pano_height * 4
        for side in ("real", "fake"):
            setattr(self, side + "_features_sum", torch.zeros(num_features, dtype=torch.float64, device=device))
            setattr(self, side + "_features_cov_sum", torch.zeros(num_features, num_features, dtype=torch.float64, device=device))
            setattr(self, side + "_features_num_samples", torch.tensor(0, dtype=torch.long, device=device))

    @classmethod
    def from_checkpoint(cls, path, pano_height=512, device="cuda", max_batch=4, trusted=False):
        """path: the reference's weights/faed.ckpt (a Lightning checkpoint: its ``state_dict`` holds ``net.encoder.*``).  Only those
        tensors are needed, so the file is read with the tensors-only unpickler; ``trusted=True`` uses the full one, for a checkpoint
        that pickles other objects next to them (hyper-parameters, callbacks) and whose source you trust: it can run code."""
        ckpt = torch.load(path, map_location="cpu", weights_only=not trusted)
        return cls(pano_height, Encoder.from_state_dict(ckpt.get("state_dict", ckpt), device=device, max_batch=max_batch))

    def get_activation(self, imgs):
        return self.encoder.features(imgs)

    @torch.no_grad()
    def update(self, imgs, real):
        features = self.get_activation(imgs).double()
        if features.shape[1] != self.num_features:
            raise ValueError("FAED: images of height %d give %d features, the metric was built for %d"
                             % (imgs.shape[2], features.shape[1], self.num_features))
        side = "real" if real else "fake"
        getattr(self, side + "_features_sum").add_(features.sum(dim=0))
        getattr(self, side + "_features_cov_sum").add_(features.t().mm(features))
        getattr(self, side + "_features_num_samples").add_(imgs.shape[0])

    def _moments(self, side):
        """The mean [d] and the unbiased covariance [d, d] of one side's features from its three states, in float64."""
        total, n = getattr(self, side + "_features_sum"), getattr(self, side + "_features_num_samples")
        mu = total / n
        return mu, (getattr(self, side + "_features_cov_sum") - n * torch.outer(mu, mu)) / (n - 1)

    def compute(self):
        """|mu_r - mu_f|^2 + tr S_r + tr S_f - 2 sum Re sqrt(eigvals(S_r S_f)), float64 (torchmetrics 1.3.2's _compute_fid)."""
        if min(int(self.real_features_num_samples), int(self.fake_features_num_samples)) < 2:
            raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
        (mu_r, s_r), (mu_f, s_f) = self._moments("real"), self._moments("fake")
        # The eigenvalues of a general matrix have no device-resident solver in torch (the GPU path is a hybrid that runs the QR
        # iteration on the host): the d x d product and its spectrum are taken on the host, in float64.
        roots = torch.linalg.eigvals(s_r.cpu() @ s_f.cpu()).sqrt().real.sum()
        return (mu_r - mu_f).square().sum() + s_r.trace() + s_f.trace() - 2 * roots.to(mu_r.device)

    def reset(self):
        for name in _STATES:
            getattr(self, name).zero_()

    def merge(self, other):
        """Add another metric's six states (another rank's, another loader's), as dist_reduce_fx="sum" does."""
        for name in _STATES:
            getattr(self, name).add_(getattr(other, name).to(getattr(self, name).device))
        return self

    def to(self, device):
        for name in _STATES:
            setattr(self, name, getattr(self, name).to(device))
        return self
