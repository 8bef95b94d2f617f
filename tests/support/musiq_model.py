"""The float64 model of ir_musiq for the tests: tools/evaluate_musiq.py run in float64 (only the input table and the standardised conv weights
keep the model's float32 roundings, which the device reads bit for bit), seeded random weights at MUSIQ's real widths (384 / 1152 / 6 heads),
the cases the tests score, the gate and the planted bugs that show what the gate can tell apart.

The gate, built as in clipiqa_model: for every case the deviation of the fp32 CPU model from the float64 model is measured - the score's
absolute deviation and the class-token feature's relative L2 deviation; the device may deviate GATE_FACTOR x the largest of them over the cases.
The device sums in another order (MFMA k-chains, fp64 statistics) and one host sample per case understates the tail of an order-dependent
error, hence the pool over the cases and the factor. Nothing is fixed in advance; the yardstick is the host model, never the kernel.
Everything here is computed once per process and shared.

Weights: GroupNorm and LayerNorm weights in [0.5, 1.5] (biases randn * 0.1), linears randn * in^-0.5 (biases randn * 0.1), the position / scale
embeddings and the class token randn * 0.5 - as large as the tokens, so that a wrong index shows. Conv weights: randn times a per-output-channel
scale spread over two decades around sqrt(1e-5), the standardisation's eps. A GroupNorm stands behind every standardised conv and removes a
factor common to a group's channels, so a wrong variance in the standardisation shows only where it moves the channels of a group by different
factors, which it does when their variances lie on both sides of that eps; the small standardised weights also keep the maps' variances near
the GroupNorms' eps, so that a wrong eps shows."""
import os
import sys

import numpy as np
import torch

from tests.support.metrics_model import ramp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import evaluate_musiq as EM  # noqa: E402

GATE_FACTOR = 8.0
HIDDEN, MLP = 384, 1152
LAYERS = {"small": 2, "real": 14}

# (name, h, w, model)
CASES = (
    ("32x32", 32, 32, "small"),        # one own-size patch; both resized scales full (7 x 7, 12 x 12); T = 195
    ("33x70", 33, 70, "small"),        # odd sizes; the 'SAME' padding split on both axes; a 2 x 3 own-size grid; T = 107
    ("45x97", 45, 97, "small"),        # T = 109
    ("100x131", 100, 131, "small"),
    ("224x160", 224, 160, "small"),    # scale 0 is a same-size resize
    ("300x500", 300, 500, "small"),    # both scales shrink; T = 292
    ("64x64_real", 64, 64, "real"),    # the 14 real layers
)
SMALL = tuple(c[0] for c in CASES if c[3] == "small")   # what the planted-bug table is evaluated on (each bug must show on at least one case)
# No case above has a resized side whose product h * ratio ends in .5, so the planted rounding bug cannot show on them. The table takes this one
# image in addition (3 * 224 / 64 = 10.5: 10 rows half-to-even, 11 half-away); it is not part of the gate.
ROUNDING_CASE = ("3x64", 3, 64, "small")
PLANTED_BUGS = EM.VARIANTS


def make_state_dict(layers, seed):
    g = torch.Generator().manual_seed(seed)
    cfg = dict(patch=EM.PATCH, hidden=HIDDEN, mlp=MLP, heads=HIDDEN // 64, layers=layers, grid=EM.GRID, longer=EM.LONGER)
    sd = {}
    for k, shape in EM.model_keys(cfg).items():
        norm = ".gn" in k or ".ln" in k or k.startswith("final_ln")
        if len(shape) == 4:
            scale = EM.STD_EPS ** 0.5 * 10.0 ** (2.0 * torch.rand((shape[0], 1, 1, 1), generator=g) - 1.5)
            sd[k] = torch.randn(shape, generator=g) * scale
        elif k in ("position_emb", "scale_emb", "cls_token"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) == 2:
            sd[k] = torch.randn(shape, generator=g) * shape[1] ** -0.5
        elif norm and k.endswith(".weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    return {k: v.float() for k, v in sd.items()}


_models = {}


def model(kind="small"):
    """The model dict of evaluate_musiq.load_model() with seeded weights."""
    if kind not in _models:
        _models[kind] = EM.load_model(make_state_dict(LAYERS[kind], 4321 if kind == "small" else 8765))
    return _models[kind]


def case(name):
    return next(c for c in CASES + (ROUNDING_CASE,) if c[0] == name)


def case_model(name):
    return model(case(name)[3])


_images = {}


def image(name):
    """The HWC uint8 image of a case: a ramp plus noise."""
    if name not in _images:
        _, h, w, _ = case(name)
        _images[name] = ramp(h, w, 3000 + 7 * [c[0] for c in CASES + (ROUNDING_CASE,)].index(name))
    return _images[name]


def run(name, dtype=torch.float64, variant=None, padding="drop"):
    """(score, class-token feature [HIDDEN] float64 array) of a case."""
    score, feat = EM.score_image(image(name), case_model(name), dtype, variant, padding)
    return score, np.asarray(feat, np.float64)


_ref, _host = {}, {}


def reference(name):
    """(score, feature) of the float64 model (computed once)."""
    if name not in _ref:
        _ref[name] = run(name)
    return _ref[name]


def deviations(score, feat, name):
    """(absolute deviation of the score, relative L2 deviation of the feature vector) from the float64 model of a case."""
    rs, rf = reference(name)
    feat = np.asarray(feat, np.float64).reshape(-1)
    return abs(float(score) - rs), float(np.linalg.norm(feat - rf) / np.linalg.norm(rf))


def host_deviation(name):
    """The fp32 CPU model's deviations on a case (computed once)."""
    if name not in _host:
        _host[name] = deviations(*run(name, torch.float32), name)
    return _host[name]


def pooled_host_deviation(names=None):
    """The largest host deviations over the cases: the yardsticks of the gate."""
    devs = [host_deviation(n) for n in (names or [c[0] for c in CASES])]
    return max(d[0] for d in devs), max(d[1] for d in devs)


def gate(names=None):
    """(score gate, feature gate)."""
    s, f = pooled_host_deviation(names)
    return GATE_FACTOR * s, GATE_FACTOR * f
