"""The float64 model of ir_dists for the tests: tools/evaluate_pairs.py::DISTS at dtype float64 (only the input table keeps the model's float32
roundings, which the device reproduces to the bit), the seeded random weights at VGG-16's real widths, the cases the tests score, the gates
and the planted bugs that show what the gates can tell apart.

The gates are measured from the reference, never from the kernel. The score lives next to 1, so its measure is the ABSOLUTE deviation from the
float64 model: the deviation of the project's fp32 host model (evaluate_pairs.DISTS on the CPU in float32) is measured per case, and the
device must stay within GATE_FACTOR x the largest of them. `40x24_flat` is ill-conditioned by definition - its variances are rounding noise
against c2 = 1e-6 - so it has a gate from its own host deviation and stays out of the pool (pooled in, it would open every case's gate by four
orders of magnitude). The moments are gated per map and moment kind: max_c |dev - ref| / max_c |ref| against GATE_FACTOR x the host model's
same measure pooled over the cases, the flat case again by itself; where the reference is exactly zero in every channel (a dead stage, the
variance of a constant image) the measure is 0 for an exact zero and infinite otherwise. Everything here is computed once per process and
shared."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.support.lpips_model import GATE_FACTOR
from tests.support.metrics_model import EP, flat, noise, ramp, shifted

CHNS = EP.DISTS_CHNS
CHANNELS = sum(CHNS)
OFFSETS = tuple(int(x) for x in np.cumsum((0,) + CHNS))
KINDS = ("mx", "my", "vx", "vy", "cxy")
WIDTHS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)   # conv k: WIDTHS[k] -> WIDTHS[k + 1]
FEATURE_IDX = tuple(i for st in EP.VGG_STAGES for i in st)
STAGE_OF = tuple(k + 1 for k, st in enumerate(EP.VGG_STAGES) for _ in st)
FLAT = "40x24_flat"

# (name, h, w, pair kind, weights)
CASES = (
    ("16x16_noise", 16, 16, "noise", "normal"),          # the maps shrink to 8, 4, 2, 1
    ("17x33_near", 17, 33, "near", "normal"),            # odd at every level: 9x17, 5x9, 3x5, 2x3 - a floor-mode pool shows
    ("35x67_noise", 35, 67, "noise", "normal"),
    ("64x64_near", 64, 64, "near", "normal"),            # +-6 per byte
    ("97x130_ramps", 97, 130, "ramps", "normal"),        # M is no multiple of a tile, several tiles
    ("64x64_dead5", 64, 64, "noise", "dead5"),           # the last conv's bias is -1e3: stage 5 is all zero, S1 = S2 = 1 from the constants alone
    ("33x18_same", 33, 18, "same", "normal"),            # b is a's copy
    (FLAT, 40, 24, "flat", "normal"),                    # both images constant, 128 and 131
    ("256x256_near", 256, 256, "near", "normal"),
    ("512x512_near", 512, 512, "near", "normal"),        # the evaluation harness's own size
)
NAMES = tuple(c[0] for c in CASES)
SMALL = NAMES[:8]   # what the planted-bug table is evaluated on (each bug must show on at least one case)


def make_weights(seed=4321, dead5=False):
    """{ir_dists_configure's names: fp32 tensors}: conv weights randn * sqrt(2 / (9 cin)), biases randn * 0.1, alpha and beta 0.01 + 0.2 * rand
    (positive as the real ones are). dead5: the last conv's bias is -1e3, so that stage 5's output is zero everywhere."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in range(13):
        cin, cout = WIDTHS[k], WIDTHS[k + 1]
        out[f"dists.c{k + 1}.w"] = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).float()
        out[f"dists.c{k + 1}.b"] = (torch.randn(cout, generator=g) * 0.1).float()
    out["dists.alpha"] = (0.01 + 0.2 * torch.rand(CHANNELS, generator=g)).float()
    out["dists.beta"] = (0.01 + 0.2 * torch.rand(CHANNELS, generator=g)).float()
    if dead5:
        out["dists.c13.b"] = torch.full_like(out["dists.c13.b"], -1e3)
    return out


def state_dicts(weights, form="module"):
    """The weights as the user's files hold them -> (model, vgg): form "module" = one state dict in the DISTS module's names (with the buffers a
    loader has to ignore), vgg None; form "vgg" = alpha / beta alone plus torchvision's `features.N.*` (with a classifier to ignore)."""
    convs = {}
    for k, (idx, st) in enumerate(zip(FEATURE_IDX, STAGE_OF)):
        base = f"stage{st}.{idx}" if form == "module" else f"features.{idx}"
        convs[base + ".weight"] = weights[f"dists.c{k + 1}.w"]
        convs[base + ".bias"] = weights[f"dists.c{k + 1}.b"]
    ab = {"alpha": weights["dists.alpha"].reshape(1, -1, 1, 1), "beta": weights["dists.beta"].reshape(1, -1, 1, 1)}
    if form == "module":
        ab.update(convs)
        ab["mean"] = torch.tensor(EP.DISTS_MEAN).view(1, -1, 1, 1)
        ab["std"] = torch.tensor(EP.DISTS_STD).view(1, -1, 1, 1)
        for st, idx, c in ((2, 4, 64), (3, 9, 128), (4, 16, 256), (5, 23, 512)):
            ab[f"stage{st}.{idx}.filter"] = torch.ones(c, 1, 3, 3) / 9
        return ab, None
    convs["classifier.0.weight"] = torch.zeros(4, 4)
    convs["classifier.0.bias"] = torch.zeros(4)
    return ab, convs


_weights, _pairs, _models, _ref, _host = {}, {}, {}, {}, {}


def weights(kind="normal"):
    if kind not in _weights:
        _weights[kind] = make_weights(dead5=kind == "dead5")
    return _weights[kind]


def case(name):
    return next(c for c in CASES if c[0] == name)


def case_weights(name):
    return weights(case(name)[4])


def pair(name):
    """(a, b) HWC uint8 of a case."""
    if name not in _pairs:
        _, h, w, kind, _ = case(name)
        seed = 2000 + 3 * NAMES.index(name)
        if kind == "noise":
            ab = noise(h, w, seed), noise(h, w, seed + 1)
        elif kind == "near":
            a = ramp(h, w, seed)
            ab = a, shifted(a, 6, seed + 1)
        elif kind == "ramps":
            ab = ramp(h, w, seed), ramp(h, w, seed + 1)[::-1, ::-1].copy()
        elif kind == "same":
            a = noise(h, w, seed)
            ab = a, a.copy()
        else:
            ab = flat(h, w, 128), flat(h, w, 131)
        _pairs[name] = ab
    return _pairs[name]


def unit(img8):
    """[1][3][h][w] float32: what evaluate_pairs.evaluate() hands to the model."""
    return torch.from_numpy(np.asarray(img8, np.float32) / 255.0).permute(2, 0, 1)[None]


def model(kind="normal", dtype=torch.float64, cls=None):
    """evaluate_pairs.DISTS (or a planted-bug subclass) with the `kind` weights."""
    key = (kind, dtype, cls)
    if key not in _models:
        ab, _ = state_dicts(weights(kind))
        _models[key] = (cls or EP.DISTS)(ab, None, "cpu", dtype)
    return _models[key]


def evaluate(name, dtype=torch.float64, cls=None):
    """(score, moments [1475][5] float64 numpy) of a case by the model."""
    a, b = pair(name)
    net = model(case(name)[4], dtype, cls)
    m = net.all_moments(unit(a), unit(b))
    return float(net.score(m)[0]), m[0].double().numpy()


def reference(name):
    """The float64 model's (score, moments) of a case (computed once)."""
    if name not in _ref:
        _ref[name] = evaluate(name)
    return _ref[name]


def host(name):
    """The fp32 host model's (score, moments) of a case (computed once)."""
    if name not in _host:
        _host[name] = evaluate(name, torch.float32)
    return _host[name]


def host_deviation(name):
    return abs(host(name)[0] - reference(name)[0])


def pooled_names():
    return tuple(n for n in NAMES if n != FLAT)


def score_gate(name):
    """The absolute gate of a case's score: pooled over every case but the flat one, which has its own."""
    if name == FLAT:
        return GATE_FACTOR * host_deviation(FLAT)
    return GATE_FACTOR * max(host_deviation(n) for n in pooled_names())


def moment_measure(m, ref):
    """[6 maps][5 kinds]: max_c |m - ref| / max_c |ref| per map and moment kind; 0 / 0 = 0, x / 0 = inf."""
    out = np.zeros((len(CHNS), 5))
    for k in range(len(CHNS)):
        sl = slice(OFFSETS[k], OFFSETS[k + 1])
        num, den = np.abs(m[sl] - ref[sl]).max(0), np.abs(ref[sl]).max(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k] = np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
    return out


def host_moment_measure(name):
    return moment_measure(host(name)[1], reference(name)[1])


def moment_gate(name):
    """[6][5]: the gate of a case's moments, pooled as the score's is."""
    if name == FLAT:
        return GATE_FACTOR * host_moment_measure(FLAT)
    return GATE_FACTOR * np.max([host_moment_measure(n) for n in pooled_names()], 0)


# ---------------------------------------------------------------------------------------------------------------- planted bugs
class _Bug(EP.DISTS):
    bug = None

    def l2pool(self, x):
        c = x.shape[1]
        if self.bug == "floor_pool":
            return super().l2pool(x)[:, :, :max(x.shape[2] // 2, 1), :max(x.shape[3] // 2, 1)]
        if self.bug == "max_pool":
            return F.max_pool2d(x, 3, 2, 1)
        if self.bug == "pool_pad0":
            x = F.pad(x, (0, max(3 - x.shape[3], 0), 0, max(3 - x.shape[2], 0)))   # a map below 3 pixels has no window without padding
            return (F.conv2d(x * x, self.window.expand(c, 1, 3, 3).contiguous(), stride=2, groups=c) + 1e-12).sqrt()
        if self.bug == "five_taps":
            a = torch.tensor(np.hanning(7)[1:-1], dtype=self.dtype)
            g = (a[:, None] * a[None, :]) / (a[:, None] * a[None, :]).sum()
            return (F.conv2d(x * x, g.expand(c, 1, 5, 5).contiguous(), stride=2, padding=2, groups=c) + 1e-12).sqrt()
        return super().l2pool(x)

    def maps(self, x01):
        if self.bug == "map0_normalised":
            return [((x01 - self.mean) / self.std).to(self.dtype)] + super().maps(x01)[1:]
        if self.bug == "tap_before_relu":
            outs = [x01.to(self.dtype)]
            h = ((x01 - self.mean) / self.std).to(self.dtype)
            for k, convs in enumerate(self.stages):
                if k:
                    h = self.l2pool(h)
                for j, (w, b) in enumerate(convs):
                    pre = F.conv2d(h, w, b, padding=1)
                    h = F.relu(pre)
                outs.append(pre)
            return outs
        return super().maps(x01)

    def moments(self, fx, fy):
        m = super().moments(fx, fy)
        if self.bug == "unbiased_variance":
            n = fx.shape[2] * fx.shape[3]
            m[..., 2:4] *= n / max(n - 1, 1)
        if self.bug == "cov_without_means":
            m[..., 4] = (fx * fy).mean((2, 3))
        return m

    def score(self, m):
        mx, my, vx, vy, cxy = m.unbind(-1)
        s1 = (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)
        s2 = (2 * cxy + 1e-6) / (vx + vy + 1e-6)
        if self.bug == "weights_not_normalised":
            return 1 - ((self.alpha * s1).sum(1) + (self.beta * s2).sum(1))
        if self.bug == "beta_on_s1":
            return 1 - ((self.beta * s1).sum(1) + (self.alpha * s2).sum(1)) / (self.alpha.sum() + self.beta.sum())
        return super().score(m)


PLANTED_BUGS = ("floor_pool", "max_pool", "pool_pad0", "five_taps", "map0_normalised", "weights_not_normalised", "unbiased_variance",
                "cov_without_means", "tap_before_relu", "beta_on_s1")
_bug_classes = {b: type("Bug_" + b, (_Bug,), {"bug": b}) for b in PLANTED_BUGS}


def bugged_score(name, bug):
    return evaluate(name, torch.float64, _bug_classes[bug])[0]
