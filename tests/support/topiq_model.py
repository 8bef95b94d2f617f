"""The float64 model of ir_topiq for the tests: tools/evaluate_topiq.py run in float64 (only the input table keeps the model's float32
roundings, which the device reads bit for bit), seeded random weights, the cases the tests score, the gate and the planted bugs that show what
the gate can tell apart.

Two seeded models. `small`: width 8, depths (2, 1, 1, 1), D = 32, 2 heads, FFN 64 - channel counts that are no tile multiple, a stage with a
block behind its first. `full`: width 64, depths (3, 4, 6, 3), D = 256, 4 heads, FFN 2048 - the shapes recalled for pyiqa's checkpoint - on one
small image.

The gate, built as in maniqa_model: for every case the deviation of the fp32 CPU model from the float64 model is measured - the score's absolute
deviation, the relative L2 deviation of feat and of each of the five level means; the device may deviate GATE_FACTOR x the largest of them over
the cases. Nothing is fixed in advance; the yardstick is the host model, never the kernel. Everything here is computed once per process.

Weights: convs and linears randn * gain * fan_in^-0.5 (gain sqrt(2) in the trunk, whose ReLUs halve the variance; biases randn * 0.1),
BatchNorm and LayerNorm weights in [0.5, 1.5], running variances in [0.5, 1.5], running means and norm biases randn * 0.1, the two position
embeddings randn * 0.5 - as large as the tokens, so that a wrong table shows. The gate's last conv is scaled by GATE_GAIN so that the sigmoid
stays inside (0.05, 0.95) for most pixels and still varies from pixel to pixel: a saturated or flat gate would let any gate conv pass."""
import os
import sys

import numpy as np
import torch

from tests.support.metrics_model import ramp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import evaluate_topiq as ET  # noqa: E402

GATE_FACTOR = 8.0
GATE_GAIN = 0.5
CONFIGS = {
    "small": dict(width=8, depths=(2, 1, 1, 1), dim=32, heads=2, ffn=64),
    "full": dict(width=64, depths=(3, 4, 6, 3), dim=256, heads=4, ffn=2048),
}
SEEDS = {"small": 8642, "full": 9753}

# (name, h, w, model)
CASES = (
    ("131x97", 131, 97, "small"),    # odd sizes at every stride; uneven adaptive bins (66 -> 5, 49 -> 4)
    ("16x200", 16, 200, "small"),    # the strip where the pool condition's AND matters: level 3 stays 1 x 13 beside 1 x 7
    ("64x64", 64, 64, "small"),      # every map is a multiple; a bin is a whole block
    ("33x40", 33, 40, "small"),      # th = 2; maps barely above the coarsest grid
    ("97x131", 97, 131, "full"),     # the real channel counts; K tails; N = 2048
)
SMALL = tuple(c[0] for c in CASES if c[3] == "small")   # what the planted-bug table is evaluated on (each bug must show on at least one case)
PLANTED_BUGS = ET.VARIANTS
PARTS = ("feat", "level0", "level1", "level2", "level3", "level4")


def make_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in ET.model_keys(cfg).items():
        if k in ("h_emb", "w_emb"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) >= 2:
            gain = 2.0 ** 0.5 if k.startswith("trunk.") else 1.0
            sd[k] = torch.randn(shape, generator=g) * gain * float(np.prod(shape[1:])) ** -0.5
        elif k.endswith("running_var") or (k.endswith(".weight") and (".bn" in k or "downsample.1" in k or ".norm" in k or k in ("score.0.weight", "score.3.weight"))):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    for i in range(5):
        sd[f"gate.{i}.conv3.weight"] = sd[f"gate.{i}.conv3.weight"] * GATE_GAIN
    return {k: v.float() for k, v in sd.items()}


_models = {}


def model(kind="small"):
    """The model dict of evaluate_topiq.load_model() with seeded weights."""
    if kind not in _models:
        cfg = CONFIGS[kind]
        _models[kind] = ET.load_model(make_state_dict(cfg, SEEDS[kind]), cfg["heads"])
        assert _models[kind]["cfg"] == {**cfg}, (_models[kind]["cfg"], cfg)
    return _models[kind]


def case(name):
    return next(c for c in CASES if c[0] == name)


def case_model(name):
    return model(case(name)[3])


_images = {}


def image(name):
    """The HWC uint8 image of a case: a ramp plus noise."""
    if name not in _images:
        _, h, w = case(name)[:3]
        _images[name] = ramp(h, w, 6000 + 7 * [c[0] for c in CASES].index(name))
    return _images[name]


def run(name, dtype=torch.float64, variant=None):
    """(score, feat [D], level means [5][D]) of a case, arrays in float64."""
    score, feat, means = ET.score_image(image(name), case_model(name), dtype, variant)
    return score, np.asarray(feat, np.float64), np.asarray(means, np.float64)


_ref, _host = {}, {}


def reference(name):
    """(score, feat, level means) of the float64 model (computed once)."""
    if name not in _ref:
        _ref[name] = run(name)
    return _ref[name]


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64).reshape(b.shape) - b) / np.linalg.norm(b))


def deviations(score, feat, means, name):
    """(absolute deviation of the score, [relative L2 deviation of feat and of each of the five level means]) from the float64 model of a case."""
    rs, rf, rm = reference(name)
    means = np.asarray(means, np.float64).reshape(rm.shape)
    return abs(float(score) - rs), [_rel(feat, rf)] + [_rel(means[i], rm[i]) for i in range(5)]


def host_deviation(name):
    """The fp32 CPU model's deviations on a case (computed once)."""
    if name not in _host:
        _host[name] = deviations(*run(name, torch.float32), name)
    return _host[name]


def pooled_host_deviation(names=None):
    """The largest host deviations over the cases: the yardsticks of the gate."""
    devs = [host_deviation(n) for n in (names or [c[0] for c in CASES])]
    return max(d[0] for d in devs), [max(d[1][k] for d in devs) for k in range(6)]


def gate(names=None):
    """(score gate, [gate of feat and of each level mean])."""
    s, f = pooled_host_deviation(names)
    return GATE_FACTOR * s, [GATE_FACTOR * v for v in f]
