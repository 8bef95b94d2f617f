"""Inputs, template and gates of the IL-NIQE tests (tests/test_ilniqe_cpu.py, tests/test_ilniqe_gpu.py). The model is tools/evaluate_ilniqe.py.

Cases: seeded RGB8 images, no fixture files - smoothed noise plus edges and a colour gradient, with no exactly flat region. Every size costs the
same 504 x 504 evaluation, so these are the smallest shapes at which each branch of the resize can go wrong: 24 x 24 (both axes enlarged),
40 x 700 (one axis shrunk with the widened kernel, one enlarged), 524 x 524 (identity weights), 600 x 1100 (both shrunk, non-integer ratios),
1048 x 1048 (exact half: NIQE's weight table). One further case has a flat 255 quarter and is used only where its test says so.

Gates. FLOORS are what the model differs by from ITSELF when its thirteen transforms per scale are taken as the dense DFT product in the
kernel's k order (evaluate_ilniqe.dft2_dense) and not with scipy.fft: the largest difference per statistic kind over the five cases, relative to
the largest magnitude of that kind within the image and scale, and of the score relative to the score; and the share of (block, plane) cells
whose table-searched alpha moves by one 0.001 step. tests/test_ilniqe_cpu.py measures them again and holds the recorded values to it. The
device's tolerances are 16 times the floors (the factor covers the MFMA's accumulation order, which the host emulation only approximates) and
the cap on alpha cells four times the measured share; a cell that moves by more than one step fails, and the counts must be equal.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import evaluate_ilniqe as EI  # noqa: E402

SIZES = {"up_24x24": (24, 24), "mixed_40x700": (40, 700), "same_524x524": (524, 524), "down_600x1100": (600, 1100), "half_1048x1048": (1048, 1048)}
FLAT = "flat_quarter_300x400"
KINDS = {"aggd": slice(30, 498), "meanvar": slice(498, 504), "weibull": slice(504, 558)}
# measured by tests/test_ilniqe_cpu.py::test_noise_floor (scipy.fft against the dense product), see docs/parity.md
FLOORS = {"aggd": 1.08e-16, "meanvar": 0.0, "weibull": 5.12e-14, "score": 1.72e-15}   # planes 4-6 pass through no transform: their floor is 0
ALPHA_SHARE = 0.0
FACTOR, ALPHA_FACTOR = 16.0, 4.0
# ir_op_dft2_f64 against scipy.fft: the floor of the transform itself, dense product against scipy.fft on seeded complex input relative to the
# largest output magnitude (measured by test_dft_floor), times the same factor
DFT_FLOOR = 1.46e-15


# The pipeline and command-line tests score images that are no case (the reduced models' outputs), so no floor was measured on them. Their
# statistics are held to the tolerances above wherever they are compared; the score is a smooth function of 468 features per block, some of
# them (the Weibull scales) a thousand times its own size, so a deviation of 8.2e-13 in a statistic may show as 1e-10 in the score. 1e-9 leaves
# that room and is six orders below what a plumbing fault shows (another rectangle, file or column moves the score by 1e-3 and more). It is
# NIQE's gate for the same tests (tests/support/niqe_model.py: SCORE_RTOL).
PLUMBING_RTOL = 1e-9


def _smooth(a, passes=2):
    for _ in range(passes):
        a = (a + np.roll(a, 1, 0) + np.roll(a, -1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 1)) / 5.0
    return a


def make(h: int, w: int, seed: int) -> np.ndarray:
    """Smoothed noise, two edges and a colour gradient; a little per-pixel noise on top keeps every region from being exactly flat."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([_smooth(rng.normal(0.0, 60.0, (h, w))) for _ in range(3)], -1) + 120.0
    img += np.stack([60.0 * xx / w, 40.0 * yy / h, 50.0 * (xx + yy) / (h + w)], -1)
    img[:, w // 3:w // 3 + max(w // 8, 1)] += 35.0
    img[h // 2:h // 2 + max(h // 6, 1)] -= 30.0
    img += rng.normal(0.0, 6.0, (h, w, 3))
    return np.clip(np.rint(img), 1, 254).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    return {name: make(h, w, 7000 + i) for i, (name, (h, w)) in enumerate(SIZES.items())}


@functools.lru_cache(maxsize=None)
def flat_case():
    img = make(300, 400, 7100).copy()
    img[:150, :200] = 255
    return img


@functools.lru_cache(maxsize=None)
def params(d: int = 40):
    """A synthetic template: seeded, d = 40, SPD covariance."""
    rng = np.random.default_rng(99)
    a = rng.normal(0.0, 1.0, (d, d))
    pv, _ = np.linalg.qr(rng.normal(0.0, 1.0, (EI.FEATURES, d)))
    return rng.normal(0.0, 1.0, d), a @ a.T / d + 0.5 * np.eye(d), rng.normal(0.0, 1.0, EI.FEATURES), pv


def write_npz(path, par=None):
    mu, cov, mean_s, pv = par or params()
    np.savez(path, mu_prisparam=mu, cov_prisparam=cov, meanOfSampleData=mean_s, principleVectors=pv)
    return str(path)


def write_mat(path, par=None):
    """ILNIQE_templateModel.mat's layout: templateModel, a 1 x 4 cell."""
    from scipy.io import savemat
    mu, cov, mean_s, pv = par or params()
    cell = np.empty((1, 4), dtype=object)
    cell[0, 0], cell[0, 1], cell[0, 2], cell[0, 3] = mu.reshape(1, -1), cov, mean_s.reshape(1, -1), pv
    savemat(str(path), {"templateModel": cell})
    return str(path)


@functools.lru_cache(maxsize=None)
def model(name: str, dft: str = "scipy"):
    """(stats [2][36][558], features [36][468], score) of a case by the model."""
    img = flat_case() if name == FLAT else cases()[name]
    stats = EI.image_stats(img, dft=dft)
    feat = EI.features_from_stats(stats)
    try:
        score = EI.score_features(feat, params())
    except ValueError:
        score = float("nan")
    for a in (stats, feat):
        a.setflags(write=False)
    return stats, feat, score


def model_score(arr) -> float:
    try:
        return EI.ilniqe(arr, params())
    except ValueError:
        return float("nan")


def kind_deviation(got: np.ndarray, want: np.ndarray, kind: str) -> float:
    """The largest |got - want| of a statistic kind relative to the largest |want| of that kind, per scale; the larger of both scales. The
    counts of the AGGD numbers are left out (they are compared for equality)."""
    worst = 0.0
    for s in range(2):
        a, b = got[s][:, KINDS[kind]], want[s][:, KINDS[kind]]
        if kind == "aggd":
            a, b = a.reshape(36, 78, 6)[..., 2:], b.reshape(36, 78, 6)[..., 2:]
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


def counts_equal(got: np.ndarray, want: np.ndarray) -> bool:
    pick = lambda st: np.concatenate([st[:, :, :30].reshape(2, 36, 5, 6)[..., :2].reshape(2, 36, -1), st[:, :, 30:498].reshape(2, 36, 78, 6)[..., :2].reshape(2, 36, -1)], -1)
    return bool(np.array_equal(pick(got), pick(want)))


def alpha_cells(got_stats: np.ndarray, want_stats: np.ndarray):
    """(cells that differ by one 0.001 step, cells that differ by more, all cells) of the table-searched alphas of plane 0's fields and planes 7-84."""
    one = more = total = 0
    for s in range(2):
        count = (EI.BLOCK // (s + 1)) ** 2
        for sl, shape in ((slice(0, 30), (36, 5, 6)), (slice(30, 498), (36, 78, 6))):
            a = EI.aggd_from_six(got_stats[s][:, sl].reshape(shape), count)[0]
            b = EI.aggd_from_six(want_stats[s][:, sl].reshape(shape), count)[0]
            steps = np.rint(np.abs(a - b) / 0.001).astype(np.int64)
            one += int((steps == 1).sum())
            more += int((steps > 1).sum())
            total += steps.size
    return one, more, total


@functools.lru_cache(maxsize=None)
def dft_input(n: int):
    """Seeded complex input (re, im) of the transform tests."""
    rng = np.random.default_rng(500 + n)
    re, im = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


@functools.lru_cache(maxsize=None)
def weibull_rows(count: int = 1764):
    """{name: row} for ir_op_weibull_fit: Weibull samples of small shape stop after one Newton step, a tight cluster with a few tiny outliers
    starts far below its shape and doubles towards it for many steps, a constant row (std(ln x) = 0, k0 = infinity) runs all fifty steps and
    ends as NaN, and so does the widest cluster-and-outlier row with a finite result or without one."""
    rng = np.random.default_rng(11)
    rows = {"one_step_k0.1": np.maximum(rng.weibull(0.1, count), 1e-300), "one_step_k0.05": np.maximum(rng.weibull(0.05, count), 1e-300),
            "two_steps_k2": rng.weibull(2.0, count), "uniform": rng.random(count) + 1e-9,
            "many_steps_a": np.concatenate([1.0 + 0.01 * rng.random(count - 4), [1e-12] * 4]),
            "many_steps_b": np.concatenate([1.0 + 0.001 * rng.random(count - 1), [1e-30]]),
            "many_steps_c": np.concatenate([1.0 + 1e-9 * rng.random(count - 1), [1e-300]]),
            "fifty_steps": np.full(count, 3.0)}
    for v in rows.values():
        v.setflags(write=False)
    return rows


def tolerance(kind: str) -> float:
    return FACTOR * FLOORS[kind]
