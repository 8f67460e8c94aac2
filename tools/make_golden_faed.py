"""Writes tests/golden/faed.npz: FAED features of two seeded image sets through the REFERENCE's own encoder with seeded weights.

Build container only (needs the reference tree; see oracle/ref_import.py).  The reference ``Encoder`` (models/faed/modules.py) is
loaded strictly with ``tests/faed_model.state_dict(SEED)``, run in float64 on ``get_activation``'s formula (FAED.py:69-78), and the
float64 model of tests/faed_model.py must reproduce it to 1e-12 before anything is written.  No weights are stored: the seed
reproduces them.

  case A  uint8 2 x 3 x 160 x 192: h' = 5, latitude weights 0, .71, 1, .71, 0
  case B  uint8 1 x 3 x 96 x 448:  w' = 14, not a multiple of any tile width
  fake_a  features of faed_model.perturb(case A, SEED): the generated side of the metric test
  e32     the reference's own float32 error against its float64 features (largest absolute difference), per case

    python tools/make_golden_faed.py
"""
import importlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import faed_model as FM  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = 2024
CASES = {"a": (2, 160, 192), "b": (1, 96, 448)}


def images(name):
    n, h, w = CASES[name]
    rng = np.random.default_rng(SEED + ord(name))
    # smooth structure plus noise, so that rows and columns differ: a low-resolution field up-sampled, then uint8
    low = rng.uniform(0, 255, (n, 3, h // 8, w // 8))
    up = np.repeat(np.repeat(low, 8, axis=2), 8, axis=3)
    return np.clip(0.7 * up + 0.3 * rng.uniform(0, 255, (n, 3, h, w)), 0, 255).astype(np.uint8)


def activation(encoder, imgs, dtype):
    """get_activation with every tensor in ``dtype``."""
    x = torch.from_numpy(imgs).type(dtype) / 127.5 - 1
    f = encoder(x)
    m = torch.mean(f, dim=3)
    weight = torch.cos(torch.linspace(math.pi / 2, -math.pi / 2, m.shape[-1], dtype=dtype)).unsqueeze(0).unsqueeze(0).expand_as(m)
    m = weight * m
    return m.reshape(-1, m.shape[-2] * m.shape[-1])


def main():
    ref_import.load()
    ref = importlib.import_module("models.faed.modules")
    sd = FM.state_dict(SEED)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    enc64, enc32 = ref.Encoder().eval().double(), ref.Encoder().eval()
    enc64.load_state_dict(tsd, strict=True)
    enc32.load_state_dict(tsd, strict=True)
    out = {"seed": np.int64(SEED)}
    with torch.no_grad():
        for name in CASES:
            imgs = images(name)
            f64 = activation(enc64, imgs, torch.float64).numpy()
            f32 = activation(enc32, imgs, torch.float32).numpy().astype(np.float64)
            mine = FM.features(sd, imgs)
            err = np.abs(mine - f64).max()
            print("case %s: features %s, |f| max %.3f, model vs reference %.2e, reference float32 error %.2e"
                  % (name, f64.shape, np.abs(f64).max(), err, np.abs(f32 - f64).max()))
            assert err <= 1e-12, err
            out["imgs_" + name], out["features_" + name] = imgs, f64
            out["e32_" + name] = np.float64(np.abs(f32 - f64).max())
        fake = activation(enc64, FM.perturb(out["imgs_a"], SEED), torch.float64).numpy()
        assert np.abs(FM.features(sd, FM.perturb(out["imgs_a"], SEED)) - fake).max() <= 1e-12
        out["features_fake_a"] = fake
    path = os.path.join(ROOT, "tests", "golden", "faed.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
