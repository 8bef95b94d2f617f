"""The float64 model of ir_clipiqa for the tests: tools/evaluate_clipiqa.py run in float64 (only the input keeps the model's float32 roundings,
which the device reproduces to the bit), seeded random weights at CLIP RN50's real width / heads / output size, the cases the tests score, the
gate and the planted bugs that show what the gate can tell apart.

The gate, built as in lpips_model: for every case the deviation of the fp32 CPU model (unfolded BatchNorm) from the float64 model is measured -
the score's absolute deviation and the feature vector's relative L2 deviation; the device may deviate GATE_FACTOR x the largest of them over
the cases. The device sums in another order (MFMA k-blocks, tiled K, folded BatchNorm, fp64 tail) and one host sample per case understates the
tail of an order-dependent error, hence the pool over the cases and the factor. Everything here is computed once per process and shared.

Text rows: with exp(logit_scale) = 100, independent random rows saturate the pair softmax at 0 / 1, which would hide errors. Each negative row is
normalize(positive + 0.5 * unit noise) instead, and reference() asserts that every pair probability of the float64 model lies in [0.02, 0.98]."""
import os
import sys

import numpy as np
import torch

from tests.support.metrics_model import ramp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import evaluate_clipiqa as EC  # noqa: E402

GATE_FACTOR = 8.0
WIDTH, OUT_DIM, PAIRS, LOGIT_SCALE_EXP = 64, 1024, 5, 100.0
LAYERS = {"small": (2, 1, 1, 2), "real": (3, 4, 6, 3)}

# (name, h, w, model)
CASES = (
    ("32x32", 32, 32, "small"),        # the last map is 1 x 1: two tokens
    ("70x45", 70, 45, "small"),        # odd extents at the stem (35 x 23), after the pool (17 x 11) and in layer 2 (8 x 5); the last map is 2 x 1
    ("63x95", 63, 95, "small"),
    ("97x130", 97, 130, "small"),
    ("256x256", 256, 256, "small"),
    ("64x64_real", 64, 64, "real"),    # the real layer counts
)
SMALL = tuple(c[0] for c in CASES[:4])   # what the planted-bug table is evaluated on (each bug must show on at least one case)
PLANTED_BUGS = EC.VARIANTS


def make_state_dict(layers, seed=4321):
    """OpenAI's `visual.*` names at the real shapes: conv weights randn * sqrt(2 / fan_in), BatchNorm weight and variance in [0.5, 1.5], bias and
    mean randn * 0.1, linears randn * in^-0.5 (their biases randn * 0.1)."""
    g = torch.Generator().manual_seed(seed)
    cfg = dict(layers=tuple(layers), width=WIDTH, heads=WIDTH * 32 // 64, out_dim=OUT_DIM)
    sd = {}
    for k, shape in EC.visual_keys(cfg).items():
        if len(shape) == 4:
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif len(shape) == 2:
            sd[k] = torch.randn(shape, generator=g) * shape[1] ** -0.5
        elif k.endswith("running_var") or (k.endswith(".weight") and "attnpool" not in k):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    return {k: v.float() for k, v in sd.items()}, cfg


def make_text(seed=99):
    """[2 PAIRS][OUT_DIM] float32 unit rows, each pair's positive row first."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(PAIRS):
        good = torch.nn.functional.normalize(torch.randn(OUT_DIM, generator=g, dtype=torch.float64), dim=0)
        unit = torch.nn.functional.normalize(torch.randn(OUT_DIM, generator=g, dtype=torch.float64), dim=0)
        rows += [good, torch.nn.functional.normalize(good + 0.5 * unit, dim=0)]
    return torch.stack(rows).float().contiguous()


_models = {}


def model(kind="small"):
    """The model dict of evaluate_clipiqa.load_model() with seeded weights."""
    if kind not in _models:
        sd, cfg = make_state_dict(LAYERS[kind], seed=4321 if kind == "small" else 8765)
        sd["logit_scale"] = torch.tensor(float(np.log(LOGIT_SCALE_EXP)))
        _models[kind] = dict(sd=sd, cfg=cfg, text=make_text(), logit_scale_exp=LOGIT_SCALE_EXP)
    return _models[kind]


def case(name):
    return next(c for c in CASES if c[0] == name)


def case_model(name):
    return model(case(name)[3])


_images = {}


def image(name):
    """The HWC uint8 image of a case: a ramp plus noise."""
    if name not in _images:
        _, h, w, _ = case(name)
        _images[name] = ramp(h, w, 2000 + 7 * [c[0] for c in CASES].index(name))
    return _images[name]


def run(name, dtype=torch.float64, variant=None, operand=None):
    """(score, feature [OUT_DIM] float64 array, pair probabilities [PAIRS]) of a case."""
    m = case_model(name)
    x = EC.scaled_input(image(name)).to(dtype)
    with torch.no_grad():
        feat = EC.image_features(x, m["sd"], m["cfg"], variant, operand)
        prob = EC.pair_probabilities(feat, m["text"], m["logit_scale_exp"], variant)
    return float(prob.double().mean()), feat[0].double().numpy(), prob[0].double().numpy()


_ref, _host, _bf16 = {}, {}, {}


def reference(name):
    """(score, feature) of the float64 model (computed once). Every pair probability lies in [0.02, 0.98]: no pair is saturated."""
    if name not in _ref:
        score, feat, prob = run(name)
        assert (prob >= 0.02).all() and (prob <= 0.98).all(), (name, prob)
        _ref[name] = (score, feat)
    return _ref[name]


def deviations(score, feat, name):
    """(absolute deviation of the score, relative L2 deviation of the feature vector) from the float64 model of a case."""
    rs, rf = reference(name)
    feat = np.asarray(feat, np.float64).reshape(-1)
    return abs(float(score) - rs), float(np.linalg.norm(feat - rf) / np.linalg.norm(rf))


def host_deviation(name):
    """The fp32 CPU model's deviations on a case (computed once)."""
    if name not in _host:
        score, feat, _ = run(name, torch.float32)
        _host[name] = deviations(score, feat, name)
    return _host[name]


def bf16_deviation(name):
    """The deviations with both operands of every convolution rounded to bf16 (fp32 accumulation): a measurement, not a gate."""
    if name not in _bf16:
        score, feat, _ = run(name, torch.float32, operand=lambda t: t.to(torch.bfloat16).to(torch.float32))
        _bf16[name] = deviations(score, feat, name)
    return _bf16[name]


def pooled_host_deviation(names=None):
    """The largest host deviations over the cases: the yardsticks of the gate."""
    devs = [host_deviation(n) for n in (names or [c[0] for c in CASES])]
    return max(d[0] for d in devs), max(d[1] for d in devs)


def gate(names=None):
    """(score gate, feature gate)."""
    s, f = pooled_host_deviation(names)
    return GATE_FACTOR * s, GATE_FACTOR * f
