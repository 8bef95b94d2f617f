"""The float64 model of ir_maniqa for the tests: tools/evaluate_maniqa.py run in float64 (only the input table keeps the model's float32
roundings, which the device reads bit for bit), seeded random weights, the cases the tests score, the gate and the planted bugs that show what
the gate can tell apart.

Two seeded models. `small`: crop 64, patch 8 (64 tokens plus class), embed 64, 2 ViT heads, ViT MLP 256, 5 ViT blocks with taps 1 .. 4 (C = 256),
window 4 (2 x 2 windows: the shift mask has all its region kinds), 2 swin heads, dim_mlp 64, scale 0.8, 5 crops - the smallest shapes at which
every kernel path can still be wrong: a token count that is no tile multiple, more than one window per axis, a shifted layer, a crop count that
is no square, C different from N so that the TAB reinterpretation is no identity. `wide`: the real widths of every kernel (crop 224, embed 768,
12 heads, MLP 3072, C = 3072, 49 windows, 4 swin heads at 192 and 96) with 4 ViT blocks, taps 0 .. 3 and ONE crop - depth adds no new shape.

The gate, built as in musiq_model: for every case the deviation of the fp32 CPU model from the float64 model is measured - the score's absolute
deviation and the head-input tokens' relative L2 deviation; the device may deviate GATE_FACTOR x the largest of them over the cases. Nothing is
fixed in advance; the yardstick is the host model, never the kernel. Everything here is computed once per process and shared.

Weights: LayerNorm weights in [0.5, 1.5] (biases randn * 0.1), linears and convs randn * in^-0.5 (biases randn * 0.1), the position embedding,
the class token and the relative-position tables randn * 0.5 - as large as the activations, so that a wrong index shows. The patch conv, the
position embedding and the class token are then scaled by INPUT_GAIN: the first block's tokens have a variance near the LayerNorm's eps, so
that a wrong eps shows. The tokens grow from stage to stage (a Swin layer enters as scale * layer(x) + x, about 1.8 x), so the heads' last
linears are scaled by HEAD_GAIN and the score head's last bias is HEAD_BIAS, so that the final ReLU and the sigmoid do not saturate: on every
case the float64 model has more than half of its per-patch scores above 0 and all weights inside (0.02, 0.98) - a condition that
tests/test_maniqa_cpu.py asserts on the reference alone; a dead head would let any trunk pass."""
import os
import sys

import numpy as np
import torch

from tests.support.metrics_model import ramp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import evaluate_maniqa as EM  # noqa: E402

GATE_FACTOR = 8.0
HEAD_GAIN, HEAD_BIAS, INPUT_GAIN = {"score": 0.003, "weight": 0.002}, 1.0, 0.01
CONFIGS = {
    "small": dict(crop=64, patch=8, embed=64, vit_heads=2, vit_mlp=256, vit_layers=5, taps=(1, 2, 3, 4), window=4, swin_heads=2, swin_depth=2, dim_mlp=64,
                  scale=0.8, crops=5),
    "wide": dict(crop=224, patch=8, embed=768, vit_heads=12, vit_mlp=3072, vit_layers=4, taps=(0, 1, 2, 3), window=4, swin_heads=4, swin_depth=2, dim_mlp=768,
                 scale=0.8, crops=1),
}
RANDOM_SEED = 77

# (name, h, w, model, crops (None: the model's), mode)
CASES = (
    ("65x65", 65, 65, "small", None, "uniform"),          # every origin is 0: all crops are equal
    ("70x131", 70, 131, "small", None, "uniform"),        # the steps differ per axis
    ("100x200", 100, 200, "small", 20, "uniform"),        # the real crop count: a 5 x 5 grid at the step of 4, the first 20
    ("97x83", 97, 83, "small", None, "random"),           # random origins from a fixed seed
    ("225x300_wide", 225, 300, "wide", None, "uniform"),  # the real widths, one crop
)
SMALL = tuple(c[0] for c in CASES if c[3] == "small")   # what the planted-bug table is evaluated on (each bug must show on at least one case)
PLANTED_BUGS = EM.VARIANTS


def make_state_dict(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in EM.model_keys(cfg).items():
        if k in ("vit.pos_embed", "vit.cls_token") or k.endswith(".rpb"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) >= 2:
            sd[k] = torch.randn(shape, generator=g) * float(np.prod(shape[1:])) ** -0.5
        elif ".ln" in k and k.endswith(".weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    for n in ("score", "weight"):
        sd[n + ".fc2.weight"] = sd[n + ".fc2.weight"] * HEAD_GAIN[n]
    sd["score.fc2.bias"] = sd["score.fc2.bias"] * 0 + HEAD_BIAS
    for k in ("vit.patch.weight", "vit.patch.bias", "vit.pos_embed", "vit.cls_token"):
        sd[k] = sd[k] * INPUT_GAIN
    return {k: v.float() for k, v in sd.items()}


_models = {}


def model(kind="small"):
    """The model dict of evaluate_maniqa.load_model() with seeded weights."""
    if kind not in _models:
        cfg = CONFIGS[kind]
        _models[kind] = EM.load_model(make_state_dict(cfg, 2468 if kind == "small" else 1357), {k: cfg[k] for k in ("taps", "scale", "crops", "vit_heads", "swin_heads")})
        assert _models[kind]["cfg"] == {**cfg}, (_models[kind]["cfg"], cfg)
    return _models[kind]


def case(name):
    return next(c for c in CASES if c[0] == name)


def case_model(name):
    return model(case(name)[3])


def origins(name):
    """[(y, x)] of a case."""
    _, h, w, kind, crops, mode = case(name)
    cfg = CONFIGS[kind]
    return EM.crop_origins(h, w, cfg["crop"], crops or cfg["crops"], mode, RANDOM_SEED, name)


_images = {}


def image(name):
    """The HWC uint8 image of a case: a ramp plus noise."""
    if name not in _images:
        _, h, w = case(name)[:3]
        _images[name] = ramp(h, w, 5000 + 7 * [c[0] for c in CASES].index(name))
    return _images[name]


def run(name, dtype=torch.float64, variant=None):
    """(score, head-input tokens [crops][N][embed / 2] float64 array, (s, w)) of a case."""
    score, feat, sw = EM.score_image(image(name), case_model(name), origins(name), dtype, variant)
    return score, np.asarray(feat, np.float64), sw


_ref, _host = {}, {}


def reference(name):
    """(score, tokens, (s, w)) of the float64 model (computed once)."""
    if name not in _ref:
        _ref[name] = run(name)
    return _ref[name]


def deviations(score, feat, name):
    """(absolute deviation of the score, relative L2 deviation of the head-input tokens) from the float64 model of a case."""
    rs, rf, _ = reference(name)
    feat = np.asarray(feat, np.float64).reshape(rf.shape)
    return abs(float(score) - rs), float(np.linalg.norm(feat - rf) / np.linalg.norm(rf))


def host_deviation(name):
    """The fp32 CPU model's deviations on a case (computed once)."""
    if name not in _host:
        _host[name] = deviations(*run(name, torch.float32)[:2], name)
    return _host[name]


def pooled_host_deviation(names=None):
    """The largest host deviations over the cases: the yardsticks of the gate."""
    devs = [host_deviation(n) for n in (names or [c[0] for c in CASES])]
    return max(d[0] for d in devs), max(d[1] for d in devs)


def gate(names=None):
    """(score gate, feature gate)."""
    s, f = pooled_host_deviation(names)
    return GATE_FACTOR * s, GATE_FACTOR * f
