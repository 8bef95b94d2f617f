"""The float64 model of ir_lpips for the tests: LPIPS v0.1 / alex as tools/evaluate_pairs.py::LPIPS defines it, restated with every step in
float64 (only the scaling layer's input keeps the model's float32 roundings, which the device reproduces to the bit), the seeded random
weights at AlexNet's real shapes, the cases the tests score, the gate and the planted bugs that show what the gate can tell apart.

The gate: for every case the relative deviation of the project's fp32 host model (evaluate_pairs.LPIPS on the CPU) from the float64 model is
measured; the device's relative deviation from the float64 model must stay within GATE_FACTOR x the largest of them. The device sums in
another order (MFMA k-blocks, tiled K, fp64 folds) and one host sample per case understates the tail of an order-dependent error, hence the
pool over the cases and the factor. Everything here is computed once per process and shared."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.support.metrics_model import EP, noise, ramp, shifted

GATE_FACTOR = 8.0
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# (name, h, w, pair kind, weights)
CASES = (
    ("31x31_noise", 31, 31, "noise", "normal"),          # every late map is 1 x 1
    ("34x31_pm6", 34, 31, "pm6", "normal"),
    ("35x67_noise", 35, 67, "noise", "normal"),          # conv1 gives 16 columns: the only pool input here that is even, so a ceil-mode pool shows
    ("64x64_near", 64, 64, "near", "normal"),
    ("97x130_ramps", 97, 130, "ramps", "normal"),
    ("64x64_dead5", 64, 64, "noise", "dead5"),           # conv5 bias -1e3: stage 5 is all zero, the 0 / (0 + 1e-10) case
    ("256x256_near", 256, 256, "near", "normal"),
    ("512x512_near", 512, 512, "near", "normal"),        # the evaluation harness's own size
)
SMALL = tuple(c[0] for c in CASES[:6])   # what the planted-bug table is evaluated on (each bug must show on at least one case)


def make_weights(seed=1234, dead5=False):
    """{ir_lpips_configure's names: fp32 tensors}: conv weights randn * sqrt(2 / (cin k k)), biases randn * 0.1, lin rand * 2 / cout (non-negative
    as the real heads are). dead5: conv5's bias is -1e3, so that its ReLU output is zero everywhere."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, (_, cin, cout, ks, _, _) in enumerate(EP.ALEX_CONVS):
        out[f"lpips.c{k + 1}.w"] = (torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5).float()
        out[f"lpips.c{k + 1}.b"] = (torch.randn(cout, generator=g) * 0.1).float()
        out[f"lpips.lin{k + 1}"] = (torch.rand(cout, generator=g) * 2.0 / cout).float()
    if dead5:
        out["lpips.c5.b"] = torch.full_like(out["lpips.c5.b"], -1e3)
    return out


def state_dicts(weights, full=False):
    """The weights as the user's files hold them: (torchvision AlexNet `features.N.*`, lpips heads `lin{k}.model.1.weight`), or with full=True one
    lpips.LPIPS().state_dict() (`net.slice*.N.*` + heads)."""
    alex, lin = {}, {}
    for k, (idx, _, cout, _, _, _) in enumerate(EP.ALEX_CONVS):
        base = EP.LPIPS_SLICE_KEY[k] if full else f"features.{idx}"
        alex[base + ".weight"] = weights[f"lpips.c{k + 1}.w"]
        alex[base + ".bias"] = weights[f"lpips.c{k + 1}.b"]
        lin[f"lin{k}.model.1.weight"] = weights[f"lpips.lin{k + 1}"].reshape(1, cout, 1, 1)
    if full:
        lin.update(alex)
        return None, lin
    return alex, lin


_weights = {}


def weights(kind="normal"):
    if kind not in _weights:
        _weights[kind] = make_weights(dead5=kind == "dead5")
    return _weights[kind]


_pairs = {}


def pair(name):
    """(a, b) HWC uint8 of a case."""
    if name not in _pairs:
        _, h, w, kind, _ = next(c for c in CASES if c[0] == name)
        seed = 1000 + 3 * [c[0] for c in CASES].index(name)
        if kind == "noise":
            ab = noise(h, w, seed), noise(h, w, seed + 1)
        elif kind == "pm6":
            a = noise(h, w, seed)
            ab = a, shifted(a, 6, seed + 1)
        elif kind == "near":
            a = ramp(h, w, seed)
            ab = a, shifted(a, 3, seed + 1)
        else:
            ab = ramp(h, w, seed), ramp(h, w, seed + 1)[::-1, ::-1].copy()
        _pairs[name] = ab
    return _pairs[name]


def case_weights(name):
    return weights(next(c for c in CASES if c[0] == name)[4])


def scaled_input(img8, normalize=True):
    """[1][3][h][w] float32: the model's network input of an HWC uint8 image, every step rounded to float32 in the model's order."""
    x = torch.from_numpy(np.asarray(img8, np.float32) / np.float32(255.0)).permute(2, 0, 1)[None]
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE).view(1, 3, 1, 1)
    x = (x - shift) / scale
    assert x.dtype == torch.float32
    return x


def lpips_f64(a8, b8, w, bug=None):
    """The float64 model. bug: None or one of PLANTED_BUGS."""
    feats = []
    for img in (a8, b8):
        x = scaled_input(img, normalize=bug != "normalize_false").double()
        outs = []
        for k, (_, _, _, _, stride, pad) in enumerate(EP.ALEX_CONVS):
            if EP.ALEX_POOL_BEFORE[k]:
                x = F.max_pool2d(x, 3, 2, ceil_mode=bug == "ceil_pool")
            if k == 0 and bug == "pad_byte0":   # the border is the byte 0 pushed through the scaling layer instead of 0 in the scaled domain
                zero = scaled_input(np.zeros((1, 1, 3), np.uint8)).double().view(1, 3, 1, 1)
                x = F.pad(x - zero, (pad, pad, pad, pad)) + zero
                pad = 0
            x = F.conv2d(x, w[f"lpips.c{k + 1}.w"].double(), w[f"lpips.c{k + 1}.b"].double(), stride=stride, padding=pad)
            if not (k == 4 and bug == "no_relu5"):
                x = F.relu(x)
            outs.append(x)
        feats.append(outs)
    total = 0.0
    for k, (xa, xb) in enumerate(zip(*feats)):
        if bug == "skip_stage3" and k == 2:
            continue
        lw = w[f"lpips.lin{4 if (bug == 'lin4_on_stage5' and k == 4) else k + 1}"].double().view(1, -1, 1, 1)
        na = xa / (xa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = xb / (xb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total += float(((na - nb) ** 2 * lw).sum(1).mean())
    return total


PLANTED_BUGS = ("pad_byte0", "ceil_pool", "normalize_false", "skip_stage3", "lin4_on_stage5", "no_relu5")


def lpips_host_fp32(a8, b8, w):
    """The project's present fp32 host model, evaluate_pairs.LPIPS on the CPU, called as evaluate_pairs.evaluate() calls it."""
    alex, lin = state_dicts(w)
    net = EP.LPIPS(alex, lin, "cpu")
    a, b = (torch.from_numpy(np.asarray(x, np.float32) / 255.0).permute(2, 0, 1)[None] for x in (a8, b8))
    return float(net(a, b, normalize=True)[0])


def rel(x, ref):
    return abs(x - ref) / abs(ref)


_ref, _host = {}, {}


def reference(name):
    """The float64 value of a case (computed once)."""
    if name not in _ref:
        _ref[name] = lpips_f64(*pair(name), case_weights(name))
    return _ref[name]


def host_deviation(name):
    """Relative deviation of the fp32 host model from the float64 model on a case (computed once)."""
    if name not in _host:
        _host[name] = rel(lpips_host_fp32(*pair(name), case_weights(name)), reference(name))
    return _host[name]


def pooled_host_deviation(names=None):
    """The largest host deviation over the cases: the yardstick of the gate."""
    return max(host_deviation(n) for n in (names or [c[0] for c in CASES]))


def gate(names=None):
    return GATE_FACTOR * pooled_host_deviation(names)
