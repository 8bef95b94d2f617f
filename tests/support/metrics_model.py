"""The host model of ir_metrics_y for the tests: tools/evaluate_pairs.py (to_y / psnr_y / ssim_y, pyiqa's definitions in numpy fp64) loaded as it is,
the inputs the tests score, and two WRONG luma variants - exact integer arithmetic and an fp32 evaluation - with the colours on which they round
differently from the model, so that a test can show that its tolerance tells them apart."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_spec = importlib.util.spec_from_file_location("evaluate_pairs", os.path.join(ROOT, "tools", "evaluate_pairs.py"))
EP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(EP)

SSIM_TOL = 1e-9   # |ssim - model|; fp64 reordering moves it by <= 5e-15, one luma off by one in a 96 x 80 pair by 1.5e-7
MSE_RTOL = 1e-9   # |mse - model| <= MSE_RTOL * max(model, 1e-8)


def _unit(img8):
    """What evaluate_pairs.evaluate() hands to the metrics: float32(v) / 255 in float32."""
    return np.asarray(img8, np.float32) / 255.0


def model_mse(a8, b8) -> float:
    d = EP.to_y(_unit(a8), 1.0) - EP.to_y(_unit(b8), 1.0)
    return float(np.mean(d * d))


def model_scores(a8, b8):
    """(mse_y, psnr_y, ssim_y) of two HWC uint8 arrays by the model."""
    a, b = _unit(a8), _unit(b8)
    return model_mse(a8, b8), EP.psnr_y(a, b), EP.ssim_y(a, b)


def within(mse, ssim, a8, b8):
    """The tolerance of every comparison with the model; returns the deviations for the assertion message."""
    m, _, s = model_scores(a8, b8)
    return abs(ssim - s) <= SSIM_TOL and abs(mse - m) <= MSE_RTOL * max(m, 1e-8), (mse, m, ssim, s)


# ---------------------------------------------------------------------------------------------------------------- inputs
def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def shifted(img, amp, seed):
    """img + an independent integer in [-amp, amp] per sample, clipped."""
    d = np.random.default_rng(seed).integers(-amp, amp + 1, img.shape)
    return np.clip(img.astype(np.int64) + d, 0, 255).astype(np.uint8)


def ramp(h, w, seed):
    """A diagonal ramp with sigma-3 noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 255.0 * (xx + yy) / max(h + w - 2, 1)], -1)
    return np.clip(np.rint(base + rng.normal(0, 3.0, base.shape)), 0, 255).astype(np.uint8)


def flat(h, w, v):
    return np.full((h, w, 3), v, np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def pairs_for(h, w, seed=0):
    """{name: (a, b)}: the input kinds of the GPU test at one size."""
    n = noise(h, w, seed + 1)
    r = ramp(h, w, seed + 2)
    cb = checkerboard(h, w)
    white = flat(h, w, 255)
    return {
        "noise_noise": (n, noise(h, w, seed + 3)),
        "noise_pm2": (n, shifted(n, 2, seed + 4)),
        "ramp_pm3": (r, shifted(r, 3, seed + 5)),
        "identical": (n, n.copy()),
        "flat_10_200": (flat(h, w, 10), flat(h, w, 200)),
        "white_black": (white, flat(h, w, 0)),
        "checker_inverse": (cb, 255 - cb),
        "white_minus_01": (white, (255 - np.random.default_rng(seed + 6).integers(0, 2, (h, w, 3))).astype(np.uint8)),
    }


# ---------------------------------------------------------------------------------------------------------------- luma variants
def luma_model(img8):
    """Rounded 255-scale luma of the model."""
    return EP.to_y(_unit(img8))


def luma_exact(img8):
    """Exact integer arithmetic: (65481 r + 128553 g + 24966 b) / 255000 + 16, rounded half to even without any floating point."""
    v = np.asarray(img8, np.int64)
    num = 65481 * v[..., 0] + 128553 * v[..., 1] + 24966 * v[..., 2] + 16 * 255000
    q, rem = np.divmod(num, 255000)
    up = (2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1))
    return (q + up).astype(np.float64)


def luma_fp32(img8):
    """The model's expression evaluated in float32 throughout."""
    x = _unit(img8)
    f = np.float32
    y = (f(16.0) + f(65.481) * x[..., 0] + f(128.553) * x[..., 1] + f(24.966) * x[..., 2]) / f(255.0) * f(255.0)
    assert y.dtype == np.float32
    return np.round(y).astype(np.float64)


def ssim_of_luma(x, y) -> float:
    """evaluate_pairs.ssim_y from the two rounded luma planes (for the variants above)."""
    g = EP._gauss_window()
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    f = EP._filter_valid
    mu1, mu2 = f(x, g), f(y, g)
    s11, s22, s12 = f(x * x, g) - mu1 * mu1, f(y * y, g) - mu2 * mu2, f(x * y, g) - mu1 * mu2
    cs = np.maximum((2 * s12 + c2) / (s11 + s22 + c2), 0.0)
    return float(np.mean((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs))


_near_tie = None


def near_tie_colours():
    """(colours where exact-integer luma rounds differently from the model, colours where the fp32 evaluation does), each [k][3] uint8, by
    enumeration of all 2^24 colours (a red plane at a time). Computed once and shared."""
    global _near_tie
    if _near_tie is None:
        gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(-1, 2).astype(np.uint8)
        exact, fp32 = [], []
        for r in range(256):
            col = np.concatenate([np.full((gb.shape[0], 1), r, np.uint8), gb], 1)[None]
            m = luma_model(col)[0]
            exact.append(col[0][luma_exact(col)[0] != m])
            fp32.append(col[0][luma_fp32(col)[0] != m])
        _near_tie = (np.concatenate(exact), np.concatenate(fp32))
    return _near_tie


def near_tie_pair(h=24, w=32, seed=11):
    """An h x w image drawn from the near-tie colours and its partner perturbed by up to +-6 per sample."""
    exact, fp32 = near_tie_colours()
    pool = np.concatenate([exact, fp32])
    rng = np.random.default_rng(seed)
    a = pool[rng.integers(0, len(pool), h * w)].reshape(h, w, 3)
    return a, shifted(a, 6, seed + 1)
