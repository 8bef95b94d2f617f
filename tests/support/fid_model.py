"""What the FID tests share: seeded weights at Inception-v3's real widths (drawn in memory, never committed), the test images, the float64 model
(tools/evaluate_fid.py::InceptionFID in fp64 on the same weights - the reference), the fp32 host model, and the gates measured from the two.

Weights: He-scaled convolutions (std = sqrt(2 / (cin kh kw))); BatchNorm weight in 0.6 .. 0.95, bias and running mean of either sign in
0.05 .. 0.3 / 0.05 .. 0.4, running variance in 0.4 .. 0.9 - away from 0 and 1, so that eps and the folding matter, with a gain near 1 per layer so
that the maps neither die nor blow up over the 47 layers of the longest path.

Gates (the margin the other scorers use): 8 x the largest deviation of the fp32 CPU model from the float64 model over the cases, measured as
max_c |f - ref| / max_c |ref| per image - for the 2048 features, and per block for the thirteen block means. The device runs an fp32 chain in
another, fixed order of additions than torch's CPU kernels; 8 x that model's own rounding distance is the accepted room for it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import evaluate_fid as EF  # noqa: E402

# name -> (h, w, seed, resize mode); the three 40x56 images are one batch of n = 3
CASES = {"299x299": (299, 299, 1, "clean"), "300x301": (300, 301, 2, "clean"), "64x48": (64, 48, 3, "clean"), "512x384": (512, 384, 4, "clean"),
         "40x56_a": (40, 56, 5, "clean"), "40x56_b": (40, 56, 6, "clean"), "40x56_c": (40, 56, 7, "clean"),
         "64x48_legacy": (64, 48, 3, "legacy"), "300x301_legacy": (300, 301, 2, "legacy")}
NAMES = list(CASES)
BATCH = ["40x56_a", "40x56_b", "40x56_c"]
OFFSETS = np.concatenate([[0], np.cumsum(EF.BLOCK_WIDTH)])
_cache = {}


def weights():
    """`fid.<name>.w / .bn_w / .bn_b / .bn_mean / .bn_var` float32 tensors, drawn once."""
    if "w" not in _cache:
        g = torch.Generator().manual_seed(20261020)

        def uni(n, lo, hi):
            return lo + (hi - lo) * torch.rand(n, generator=g)

        def signed(n, lo, hi):
            return uni(n, lo, hi) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
        out = {}
        for name, cin, cout, kh, kw, _, _, _ in EF.CONVS:
            out[f"fid.{name}.w"] = torch.randn((cout, cin, kh, kw), generator=g) * float(np.sqrt(2.0 / (cin * kh * kw)))
            out[f"fid.{name}.bn_w"] = uni(cout, 0.6, 0.95)
            out[f"fid.{name}.bn_b"] = signed(cout, 0.05, 0.3)
            out[f"fid.{name}.bn_mean"] = signed(cout, 0.05, 0.4)
            out[f"fid.{name}.bn_var"] = uni(cout, 0.4, 0.9)
        _cache["w"] = {k: v.to(torch.float32).contiguous() for k, v in out.items()}
    return _cache["w"]


def state_dict():
    """The same weights under pytorch-fid / torchvision names, with the keys a real file has besides (they are ignored)."""
    w = weights()
    sd = {}
    for name, *_ in EF.CONVS:
        sd[f"{name}.conv.weight"] = w[f"fid.{name}.w"]
        for mine, theirs in EF.BN_PARTS:
            sd[f"{name}.{theirs}"] = w[f"fid.{name}.{mine}"]
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    sd["fc.weight"] = torch.zeros((1008, 2048))
    sd["fc.bias"] = torch.zeros((1008,))
    sd["AuxLogits.conv0.conv.weight"] = torch.zeros((128, 768, 1, 1))
    return sd


def image(name):
    """[h][w][3] uint8: smooth structure plus noise, so that both the resize and the network see something."""
    h, w, seed, _ = CASES[name]
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 90 * np.sin(xx / (3.0 + c) + seed) * np.cos(yy / (5.0 - c) + c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def model(dtype="fp64", **variant):
    key = ("model", dtype, tuple(sorted(variant.items())))
    if key not in _cache:
        _cache[key] = EF.InceptionFID(weights(), dtype, **variant)
    return _cache[key]


def _run(name, dtype):
    key = ("run", name, dtype)
    if key not in _cache:
        f, means = model(dtype).features(EF.network_input(image(name), CASES[name][3])[None])
        _cache[key] = f[0], np.concatenate([m[0] for m in means])
    return _cache[key]


def reference(name):
    """(features [2048], block means [10304]) of the float64 model."""
    return _run(name, "fp64")


def host(name):
    """The same of the fp32 host model."""
    return _run(name, "fp32")


def measure(f, ref):
    """max_c |f - ref| / max_c |ref|"""
    return float(np.abs(np.asarray(f, np.float64) - ref).max() / np.abs(ref).max())


def block_measure(means, ref):
    return np.array([measure(means[OFFSETS[k]:OFFSETS[k + 1]], ref[OFFSETS[k]:OFFSETS[k + 1]]) for k in range(len(EF.BLOCKS))])


def host_deviation():
    """(the fp32 host model's largest feature deviation over the cases, the same per block [13])"""
    if "dev" not in _cache:
        _cache["dev"] = (max(measure(host(n)[0], reference(n)[0]) for n in NAMES), np.max([block_measure(host(n)[1], reference(n)[1]) for n in NAMES], 0))
    return _cache["dev"]


def feature_gate():
    return 8.0 * host_deviation()[0]


def block_gates():
    return 8.0 * host_deviation()[1]
