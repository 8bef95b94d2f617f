#!/usr/bin/env python3
"""NIQE of an output folder: the one no-reference metric of the reference's evaluate_img.py that is no pretrained network (`create_metric('niqe')`
next to MANIQA / MUSIQ / CLIPIQA, which are; tools/evaluate_maniqa.py, tools/evaluate_musiq.py and tools/evaluate_clipiqa.py score those).

    python tools/evaluate_niqe.py -i results/ --niqe_params niqe_modelparameters.mat [--ntest N] [--backend gpu]

The reference takes it from pyiqa, which is not in this image; the reference tree holds no NIQE code of its own. So the definition is RESTATED
here in plain numpy fp64 from the published implementations (pyiqa's `niqe` defaults: Y of YIQ, crop_border 0, 96 x 96 blocks) - parity with
pyiqa itself is unpinned until a box that has it runs tools/repin_with_diffusers.py. The pristine parameters (`mu_prisparam` [36],
`cov_prisparam` [36][36]: pyiqa's niqe_modelparameters.mat, a few KB) do not exist offline either: the user passes them, as a .mat or an .npz.

The definition is fixed down to the ORDER OF ADDITIONS, and this file is the model ir_niqe_stats (csrc/niqe.hip) is tested against. On an
exactly flat area (saturated sky) y - mu is pure rounding noise, and its sign decides which side of the asymmetric fit every pixel of the area
counts on: a 2-D 49-tap sum and a separable 7 + 7 sum give opposite signs on a whole flat 255 patch and move the score of a 192 x 288 image by
0.2 %. pyiqa inherits whatever order its convolution happens to use; this model and the kernel agree on one:
  1. luma: x_c = float64(float32(v) / float32(255)); y = rint(((0.299 x_r + 0.587 x_g) + 0.114 x_b) * 255), an integer 0 .. 255. Only the
     top-left (h // 96 * 96) x (w // 96 * 96) rectangle is used.
  2. window: 7 x 7, exp(-(i^2 + j^2) / (2 (7/6)^2)), entries below eps * max zeroed, divided by its sum. The library's table
     (ir_niqe_window) is the authoritative one and is read when the library has been built; the formula here agrees with it within 1 ulp.
  3. MSCN: replicate padding; mu = sum k[i][j] y[r + i - 3][c + j - 3] from 0.0 in row-major tap order, one multiply and one add per tap; m2
     the same over y y; sigma = sqrt(|m2 - mu mu|); m = (y - mu) / (sigma + 1).
  4. scale 2: y2 = half(y / 255.0) * 255.0, half = MATLAB's antialiased bicubic imresize(., 0.5): output o takes inputs 2o - 3 .. 2o + 4 with
     (-3, -9, 29, 111, 111, 29, -9, -3) / 256, symmetric padding, down the columns first (h -> h / 2), then along the rows, each pass summed
     from 0.0 over taps 0 .. 7.
  5. blocks of B = 96 / scale, row-major: p0 = m, p_s = m * roll(m, (di, dj)) INSIDE the block for (0,1), (1,0), (1,1), (1,-1); of each field
     count(p < 0), count(p > 0), sum p^2 over the negatives, over the positives, sum |p|, sum p^2.
  6. the asymmetric generalised Gaussian fit from those six numbers (aggd_features), 18 features per block and scale, 36 per block.
  7. mu_d = column means over the non-NaN entries, cov_d = unbiased covariance of the rows without NaN,
     sqrt(d pinv((cov_pris + cov_d) / 2) d^T), d = mu_pris - mu_d. Fewer than two complete rows: no score (ValueError).
Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import ctypes
import math
import os
import sys
from pathlib import Path

import numpy as np

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
HALF_WEIGHTS = np.array([-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0]) / 256.0   # exactly dyadic; sum 1.0
_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "instarevive_amd", "csrc", "libinstarevive_hip.so")


def window_formula() -> np.ndarray:
    """The window by the formula, evaluated with libm's exp and summed in row-major order."""
    g = np.array([[math.exp(-((i - 3.0) ** 2 + (j - 3.0) ** 2) / (2.0 * (7.0 / 6.0) ** 2)) for j in range(7)] for i in range(7)])
    g[g < np.finfo(np.float64).eps * g.max()] = 0.0
    total = 0.0
    for v in g.reshape(-1):
        total += float(v)
    return g / total


def window() -> np.ndarray:
    """The 7 x 7 window: the library's own 49 doubles when it has been built (so that model and kernel multiply by the same bits), the formula
    otherwise."""
    path = os.environ.get("INSTAREVIVE_HIP_LIB") or _LIB
    if os.path.exists(path):
        lib = ctypes.CDLL(path)
        if hasattr(lib, "ir_niqe_window"):
            buf = (ctypes.c_double * 49)()
            if lib.ir_niqe_window(buf) == 0:
                return np.array(buf, dtype=np.float64).reshape(7, 7)
    return window_formula()


def luma(img8: np.ndarray) -> np.ndarray:
    """Step 1 on the scored rectangle of an HWC uint8 RGB array."""
    img8 = np.asarray(img8)
    h, w = img8.shape[0] // BLOCK * BLOCK, img8.shape[1] // BLOCK * BLOCK
    x = (img8[:h, :w].astype(np.float32) / np.float32(255.0)).astype(np.float64)
    return np.rint(((0.299 * x[..., 0] + 0.587 * x[..., 1]) + 0.114 * x[..., 2]) * 255.0)


def mscn(y: np.ndarray, k: np.ndarray, pad_mode: str = "edge", separable: bool = False) -> np.ndarray:
    """Step 3. pad_mode / separable exist for the tests' planted bugs."""
    h, w = y.shape
    yp = np.pad(y, 3, mode=pad_mode) if pad_mode != "zero" else np.pad(y, 3, mode="constant")
    sq = yp * yp
    if separable:   # a 7 + 7 sum with the window's own 1-D factor: the order a separable convolution would use
        g = np.sqrt(np.diag(k))

        def sep(p):
            t = np.zeros((h + 6, w))
            for j in range(7):
                t = t + g[j] * p[:, j:j + w]
            o = np.zeros((h, w))
            for i in range(7):
                o = o + g[i] * t[i:i + h]
            return o
        mu, m2 = sep(yp), sep(sq)
    else:
        mu, m2 = np.zeros((h, w)), np.zeros((h, w))
        for i in range(7):
            for j in range(7):
                mu = mu + k[i, j] * yp[i:i + h, j:j + w]
                m2 = m2 + k[i, j] * sq[i:i + h, j:j + w]
    sigma = np.sqrt(np.abs(m2 - mu * mu))
    return (y - mu) / (sigma + 1.0)


def _half_axis0(x: np.ndarray, pad_mode: str) -> np.ndarray:
    n = x.shape[0] // 2
    xp = np.pad(x, ((3, 3), (0, 0)), mode=pad_mode)
    out = np.zeros((n, x.shape[1]))
    for t in range(8):
        out = out + HALF_WEIGHTS[t] * xp[t:t + 2 * n:2]
    return out


def half(x: np.ndarray, pad_mode: str = "symmetric", columns_first: bool = True) -> np.ndarray:
    """Step 4's imresize(., 0.5): down the columns (axis 0) first, then along the rows."""
    if columns_first:
        return _half_axis0(_half_axis0(x, pad_mode).T, pad_mode).T
    return _half_axis0(_half_axis0(x.T, pad_mode).T, pad_mode)


def scale_planes(img8: np.ndarray, **variant):
    """(y, y2): the luma plane and the half-size plane (steps 1 and 4)."""
    y = luma(img8)
    unit = np.arange(256, dtype=np.float64) / 255.0
    hv = {k: v for k, v in variant.items() if k in ("pad_mode", "columns_first")}
    return y, half(unit[y.astype(np.int64)], **hv) * 255.0


def block_stats(m: np.ndarray, b: int, circular: bool = True, shifts=SHIFTS) -> np.ndarray:
    """Step 5: [blocks][5][6] of an MSCN plane."""
    by, bx = m.shape[0] // b, m.shape[1] // b
    out = np.zeros((by * bx, 5, 6))
    for r in range(by):
        for c in range(bx):
            blk = m[r * b:(r + 1) * b, c * b:(c + 1) * b]
            fields = [blk]
            for di, dj in shifts:
                if circular:
                    fields.append(blk * np.roll(blk, (di, dj), axis=(0, 1)))
                else:   # planted bug: the roll runs over the whole plane
                    fields.append(blk * np.roll(m, (di, dj), axis=(0, 1))[r * b:(r + 1) * b, c * b:(c + 1) * b])
            for f, p in enumerate(fields):
                neg, pos, sq = p < 0, p > 0, p * p
                out[r * bx + c, f] = (neg.sum(), pos.sum(), sq[neg].sum(), sq[pos].sum(), np.abs(p).sum(), sq.sum())
    return out


def image_stats(img8: np.ndarray, k: np.ndarray = None, **variant) -> np.ndarray:
    """Steps 1-5: [2][blocks][5][6], what ir_niqe_stats writes for one image. variant: the planted bugs of tests/test_niqe_cpu.py."""
    k = window() if k is None else k
    y, y2 = scale_planes(img8, **variant)
    if y.shape[0] < BLOCK or y.shape[1] < BLOCK:
        raise ValueError("NIQE needs at least one 96 x 96 block")
    mv = {kk: v for kk, v in variant.items() if kk in ("separable",)}
    if "mscn_pad" in variant:
        mv["pad_mode"] = variant["mscn_pad"]
    bv = {kk: v for kk, v in variant.items() if kk in ("circular", "shifts")}
    return np.stack([block_stats(mscn(y, k, **mv), BLOCK, **bv), block_stats(mscn(y2, k, **mv), BLOCK // 2, **bv)])


_gam = None


def gam_table():
    """(gam, r_gam): gam = arange(0.2, 10.001, 0.001), r_gam = Gamma(2/g)^2 / (Gamma(1/g) Gamma(3/g)), strictly increasing."""
    global _gam
    if _gam is None:
        gam = np.arange(0.2, 10.001, 0.001)
        r = np.array([math.exp(2.0 * math.lgamma(2.0 / g) - math.lgamma(1.0 / g) - math.lgamma(3.0 / g)) for g in gam])
        _gam = (gam, r)
    return _gam


def aggd_rn(six: np.ndarray, b: int):
    """(ls, rs, rn) of one field's six numbers."""
    cl, cr, sl, sr, sa, ss = (float(v) for v in six)
    with np.errstate(all="ignore"):
        ls = np.sqrt(np.float64(sl) / np.float64(cl))
        rs = np.sqrt(np.float64(sr) / np.float64(cr))
        g = ls / rs
        n = float(b * b)
        rhat = (np.float64(sa) / n) ** 2 / (np.float64(ss) / n)
        rn = rhat * (g ** 3 + 1.0) * (g + 1.0) / (g ** 2 + 1.0) ** 2
    return ls, rs, rn


def aggd(six: np.ndarray, b: int):
    """(alpha, beta_l, beta_r): step 6 for one field. The first minimum of |r_gam - rn| wins; a NaN rn takes entry 0, as argmin does."""
    gam, r_gam = gam_table()
    ls, rs, rn = aggd_rn(six, b)
    alpha = float(gam[int(np.argmin(np.abs(r_gam - rn)))])
    with np.errstate(all="ignore"):
        scale = math.sqrt(math.exp(math.lgamma(1.0 / alpha) - math.lgamma(3.0 / alpha)))
        return alpha, ls * scale, rs * scale


def block_features(stats: np.ndarray) -> np.ndarray:
    """Step 6: [2][blocks][5][6] -> [blocks][36]."""
    nb = stats.shape[1]
    feat = np.zeros((nb, 36))
    for s in range(2):
        b = BLOCK // (s + 1)
        for i in range(nb):
            row = []
            for f in range(5):
                alpha, bl, br = aggd(stats[s, i, f], b)
                if f == 0:
                    row += [alpha, (bl + br) / 2.0]
                else:
                    row += [alpha, (br - bl) * math.exp(math.lgamma(2.0 / alpha) - math.lgamma(1.0 / alpha)), bl, br]
            feat[i, 18 * s:18 * s + 18] = row
    return feat


def score_features(feat: np.ndarray, mu_pris: np.ndarray, cov_pris: np.ndarray, biased: bool = False) -> float:
    """Step 7."""
    feat = np.asarray(feat, np.float64)
    ok = ~np.isnan(feat).any(axis=1)
    if int(ok.sum()) < 2:
        raise ValueError("NIQE needs two feature rows without NaN")
    cnt = (~np.isnan(feat)).sum(axis=0)
    mu_d = np.where(np.isnan(feat), 0.0, feat).sum(axis=0) / cnt
    rows = feat[ok]
    cen = rows - rows.mean(axis=0)
    cov_d = cen.T @ cen / (rows.shape[0] - (0 if biased else 1))
    d = (np.asarray(mu_pris, np.float64).reshape(1, 36) - mu_d.reshape(1, 36))
    inv = np.linalg.pinv((np.asarray(cov_pris, np.float64) + cov_d) / 2.0)
    return float(np.sqrt((d @ inv @ d.T)[0, 0]))


def niqe(img8: np.ndarray, mu_pris, cov_pris, k: np.ndarray = None, **variant) -> float:
    biased = variant.pop("biased", False)
    return score_features(block_features(image_stats(img8, k, **variant)), mu_pris, cov_pris, biased=biased)


def load_params(path):
    """(mu_prisparam [36], cov_prisparam [36][36]) of a .mat (scipy.io.loadmat) or an .npz."""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
    else:
        from scipy.io import loadmat
        d = loadmat(str(path))
    if "mu_prisparam" not in d or "cov_prisparam" not in d:
        raise ValueError(f"{path}: mu_prisparam / cov_prisparam missing")
    mu, cov = np.asarray(d["mu_prisparam"], np.float64).reshape(-1), np.asarray(d["cov_prisparam"], np.float64)
    if mu.shape != (36,) or cov.shape != (36, 36):
        raise ValueError(f"{path}: mu_prisparam {mu.shape} / cov_prisparam {cov.shape} are not 36 and 36 x 36")
    return mu, cov


def evaluate(img_dir, params, ntest=None, backend="host", log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    mu, cov = load_params(params)
    ctx = nq = None
    if backend == "gpu":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from instarevive_amd import _lib as L, niqe as nq
        ctx = L.Context(0)
    k = window()
    total, scored, skipped = 0.0, 0, 0
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            v = nq.score_arrays(ctx, img, (mu, cov)) if ctx is not None else niqe(img, mu, cov, k)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"niqe: {total / scored:.5f}")
    return total / scored if scored else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--niqe_params", required=True, help="niqe_modelparameters.mat (pyiqa's) or an .npz with mu_prisparam / cov_prisparam")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    evaluate(a.img_path, a.niqe_params, a.ntest, backend=a.backend)


if __name__ == "__main__":
    main()
