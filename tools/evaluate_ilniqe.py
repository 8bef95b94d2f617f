#!/usr/bin/env python3
"""IL-NIQE of an output folder: the no-reference metric that the reference's evaluate_img.py keeps commented out next to `niqe`
(`# metric_dict["ilniqe"] = pyiqa.create_metric('ilniqe')`), and like NIQE classical statistics against a small pristine model, no network.

    python tools/evaluate_ilniqe.py -i results/ --ilniqe_params ILNIQE_templateModel.mat [--ntest N] [--backend host|gpu]

pyiqa is not in this image and neither is the template file, so the definition (Zhang, Zhang and Bovik 2015, the MATLAB release as pyiqa's
`ilniqe` restates it) is RESTATED here in plain numpy / scipy fp64. Where MATLAB and pyiqa may differ, MATLAB is taken; parity with pyiqa is
unpinned (docs/parity.md) until a box that has it runs tools/repin_with_diffusers.py. The user passes the template: a .mat with the 1 x 4 cell
`templateModel` = (mu_prisparam [d], cov_prisparam [d][d], meanOfSampleData [468], principleVectors [468][d]) or an .npz with those four names.
This file is the model the device code (csrc/ilniqe.hip: ir_ilniqe_stats, ir_op_dft2_f64, ir_op_weibull_fit) is tested against; `--backend gpu`
scores through it (instarevive_amd/ilniqe.py). The tables (windows, taps, filters, resize weights) are made here in fp64 exactly as
instarevive_amd/ilniqe.py and the library's ir_ilniqe_plan make them: the tests compare the bits.

Constants: normalised size 524, block 84, sigmaForGauDerivative 1.66, KforLog 1e-5, minWaveLength 2.4, sigmaOnf 0.55, mult 1.31,
dThetaOnSigma 1.10, scaleFactorForLoG 0.87, scaleFactorForGaussianDer 0.28, sigmaForDownsample 0.9, EPS 1e-8, 3 log-Gabor scales,
4 orientations, infConst 10000.

  1. resize: x = float64(v) on 0 .. 255; MATLAB's antialiased bicubic imresize (a = -0.5) to 524 x 524: scale = out / in, the kernel is widened
     by 1 / scale when scale < 1 (h(t) = scale cubic(scale t)), P = ceil(width) + 2 taps from left = floor(u - width / 2) with
     u = o / scale + 0.5 (1 - 1 / scale) (o 1-based), weights divided by their sum (added from 0.0 in tap order), symmetric padding; down the
     columns first, then along the rows, each output summed from 0.0 in tap order; clamped to [0, 255]. The top-left 504 x 504 (6 x 6 blocks
     of 84) is used.
  2. opponent planes: O1 = (0.3 R + 0.04 G) - 0.35 B, O2 = (0.34 R - 0.6 G) + 0.17 B, O3 = (0.06 R + 0.63 G) + 0.27 B.
  3. per scale s = 1, 2 (blocks of 84 / s, 36 blocks at both), 109 planes:
       0        MSCN of O3: 5 x 5 window fspecial('gaussian', 5, 5/6) (entries below eps * max zeroed, divided by the sum), replicate padding,
                mu and m2 as 25-tap sums from 0.0 in row-major tap order with separate multiplies and adds, m = (O3 - mu) / (sqrt(|m2 - mu mu|) + 1)
       1-3      GM = sqrt(Ix^2 + Iy^2 + EPS) of O1, O2, O3. Ix, Iy = conv2(., 'same') (a true convolution, zero padding) with
                x exp(-(x^2 + y^2) / (2 sg^2)) and y exp(..) on -L .. L, L = ceil(3 sg), sg = 1.66 / s^0.28 (11 x 11 at both scales). The kernels
                are rank one and are applied as two 11-tap passes: along the rows (x) first, then down the columns (y), each from 0.0 in tap order.
       4-6      l_c = log(c + 1e-5) - mean(log(c + 1e-5)) for c = R, G, B, with log as det_log() states it and the plane's sum in the order of
                wg_sum(., 1024); (r + g + b) / sqrt 3, (r + g - 2 b) / sqrt 6, (r - g) / sqrt 2
       7-12     Ix(O1), Iy(O1), Ix(O2), Iy(O2), Ix(O3), Iy(O3)
       13-36    for the 12 log-Gabor filters in (scale, orientation) order, f = 4 k + o: Re, Im of ifft2(F_f .* fft2(O3))
       37-84    per filter f: dx Re, dy Re, dx Im, dy Im (the same derivative kernels)
       85-108   per filter f: sqrt(dxRe^2 + dyRe^2) + EPS, sqrt(dxIm^2 + dyIm^2) + EPS
     filters: Kovesi's log-Gabor times angular spread on the ifftshifted frequency grid of the plane's size (x = (-N/2 .. N/2 - 1) / N for even N),
     radius(0,0) = 1, theta = atan2(-y, x); wavelengths (2.4 / s^0.87) 1.31^k, radial part exp(-log(r / f0)^2 / (2 log(0.55)^2)) times the
     low-pass 1 / (1 + (r / 0.45)^30), DC zeroed; spread exp(-dtheta^2 / (2 thetaSigma^2)), thetaSigma = pi / 4 / 1.10,
     dtheta = |atan2(sin(theta - a), cos(theta - a))| through the expanded products, a = o pi / 4.
     between scales: O1 .. O3 and R, G, B are filtered with the 6 x 6 fspecial('gaussian', 6, 0.9) as MATLAB's imfilter does (correlation,
     replicate padding, centre at index 2 of 0 .. 5: taps -2 .. +3, a 36-tap sum from 0.0 in row-major order) and rows / columns 0, 2, 4, ...
     are kept: 252 x 252.
  4. per block and scale 234 features: plane 0 - the AGGD fit (NIQE's, from the six numbers count(p < 0), count(p > 0), sum p^2 over either side,
     sum |p|, sum p^2; every sum of a block in the order of wg_sum()) gives alpha, (beta_l + beta_r) / 2, and the four products with the copy shifted circularly inside the block by (0,1),
     (1,0), (1,1), (1,-1) give alpha, mean, beta_l, beta_r (18); planes 1-3 - the Weibull fit as (scale, shape) = (lambda, k) (6); planes 4-6 -
     mean and unbiased variance (6); planes 7-84 - alpha, (beta_l + beta_r) / 2 (156); planes 85-108 - Weibull (48). Weibull: l = ln x,
     k0 = 1.2 / std(l) (unbiased), Newton on f(k) = sum(x^k l) / sum(x^k) - mean(l) - 1 / k with x^k = exp(k l) and
     f'(k) = sum(x^k l^2) / sum(x^k) - (sum(x^k l) / sum(x^k))^2 + 1 / k^2, at most 50 steps, stop when |k - k_prev| < 1e-2,
     lambda = mean(x^k)^(1 / k). 468 features per block, scale 1 first.
  5. score: values above 10000 are set to 10000; c = P^T (f - meanOfSampleData) per block; mu_d the nan-mean over blocks, blocks with NaN take mu_d
     in those entries; cov_d the unbiased covariance over the blocks without NaN; q = sqrt(d pinv((cov_pris + cov_d) / 2) d^T), d = c - mu_pris,
     per block; the score is the mean of q. Fewer than two complete blocks: no score (ValueError).
The statistics of one image are [2][36][558] doubles per scale and block: 5 x 6 AGGD numbers of plane 0's fields, 78 x 6 of planes 7-84,
3 x (mean, variance) of planes 4-6, 27 x (k, lambda) of planes 1-3 and 85-108.
Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import math
import os
import sys
from pathlib import Path

import numpy as np

SIZE, BLOCK, USED = 524, 84, 504
EPS, K_LOG, INF_CONST = 1e-8, 1e-5, 10000.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
STATS = 30 + 78 * 6 + 6 + 54
FEATURES = 468
WEIBULL_STEPS, WEIBULL_TOL = 50, 1e-2


# ---------------------------------------------------------------------------------------------------------------- step 1
def _cubic(x):
    a = np.abs(x)
    return np.where(a <= 1.0, (1.5 * a - 2.5) * a * a + 1.0, np.where(a <= 2.0, ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0, 0.0))


def resize_weights(n_in: int, n_out: int):
    """(index [n_out][P] int64, 0-based and symmetric-padded; weight [n_out][P]) of MATLAB's antialiased bicubic imresize along one axis."""
    scale = n_out / n_in
    width = 4.0 / scale if scale < 1.0 else 4.0
    taps = int(math.ceil(width)) + 2
    u = np.arange(1, n_out + 1) / scale + 0.5 * (1.0 - 1.0 / scale)
    left = np.floor(u - width / 2.0)
    idx = left[:, None] + np.arange(taps)[None, :]          # 1-based
    d = u[:, None] - idx
    w = scale * _cubic(scale * d) if scale < 1.0 else _cubic(d)
    total = np.zeros(n_out)
    for t in range(taps):
        total = total + w[:, t]
    w = w / total[:, None]
    aux = np.concatenate([np.arange(n_in), np.arange(n_in - 1, -1, -1)])
    return aux[np.mod(idx.astype(np.int64) - 1, 2 * n_in)], w


def _resize_axis0(x, n_out):
    idx, w = resize_weights(x.shape[0], n_out)
    out = np.zeros((n_out,) + x.shape[1:])
    for t in range(idx.shape[1]):
        out = out + w[:, t].reshape((-1,) + (1,) * (x.ndim - 1)) * x[idx[:, t]]
    return out


def resize524(img8: np.ndarray) -> np.ndarray:
    """Step 1: HWC uint8 RGB -> [504][504][3] float64."""
    x = np.asarray(img8).astype(np.float64)
    x = _resize_axis0(x, SIZE)
    x = np.swapaxes(_resize_axis0(np.swapaxes(x, 0, 1), SIZE), 0, 1)
    return np.clip(x, 0.0, 255.0)[:USED, :USED]


# ---------------------------------------------------------------------------------------------------------------- tables
def gaussian_window(size: int, sigma: float) -> np.ndarray:
    """MATLAB's fspecial('gaussian', size, sigma), summed in row-major order."""
    c = (size - 1) / 2.0
    g = np.array([[math.exp(-((i - c) ** 2 + (j - c) ** 2) / (2.0 * sigma * sigma)) for j in range(size)] for i in range(size)])
    g[g < np.finfo(np.float64).eps * g.max()] = 0.0
    total = 0.0
    for v in g.reshape(-1):
        total += float(v)
    return g / total


def derivative_taps(scale: int):
    """(x g(x), g(x)) on -L .. L for sg = 1.66 / scale^0.28: dx's kernel is outer(g, xg) (x along the columns), dy's outer(xg, g)."""
    sg = 1.66 / scale ** 0.28
    half = int(math.ceil(3.0 * sg))
    g = np.array([math.exp(-(t * t) / (2.0 * sg * sg)) for t in range(-half, half + 1)])
    return np.arange(-half, half + 1) * g, g


def log_gabor_bank(n: int, scale: int) -> np.ndarray:
    """[12][n][n] real filters in (scale, orientation) order on the ifftshifted grid."""
    r = (np.arange(-(n // 2), n - n // 2) / n) if n % 2 == 0 else (np.arange(-(n - 1) // 2, (n - 1) // 2 + 1) / (n - 1))
    x, y = np.meshgrid(r, r)
    radius = np.fft.ifftshift(np.sqrt(x * x + y * y))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    lp = 1.0 / (1.0 + (radius / 0.45) ** 30)
    radius[0, 0] = 1.0
    sin_t, cos_t = np.sin(theta), np.cos(theta)
    theta_sigma = math.pi / 4 / 1.10
    bank = np.zeros((12, n, n))
    for k in range(3):
        f0 = 1.0 / ((2.4 / scale ** 0.87) * 1.31 ** k)
        radial = np.exp(-np.log(radius / f0) ** 2 / (2.0 * math.log(0.55) ** 2)) * lp
        radial[0, 0] = 0.0
        for o in range(4):
            a = o * math.pi / 4
            ds = sin_t * math.cos(a) - cos_t * math.sin(a)
            dc = cos_t * math.cos(a) + sin_t * math.sin(a)
            dtheta = np.abs(np.arctan2(ds, dc))
            bank[4 * k + o] = radial * np.exp(-dtheta ** 2 / (2.0 * theta_sigma ** 2))
    return bank


_twiddles = {}


def twiddles(n: int):
    """(cos, sin) of 2 pi (jk mod n) / n as [n][n], evaluated with libm as the library's host code does."""
    if n not in _twiddles:
        jk = np.outer(np.arange(n), np.arange(n)) % n
        vals_c = np.array([math.cos(2.0 * math.pi * v / n) for v in range(n)])
        vals_s = np.array([math.sin(2.0 * math.pi * v / n) for v in range(n)])
        _twiddles[n] = (vals_c[jk], vals_s[jk])
    return _twiddles[n]


def _cgemm_k4(ar, ai, br, bi):
    """The complex product in the kernel's k order: steps of four, real part Are Bre then -Aim Bim, imaginary part Aim Bre then Are Bim."""
    n = ar.shape[1]
    re, im = np.zeros((ar.shape[0], br.shape[1])), np.zeros((ar.shape[0], br.shape[1]))
    for k in range(0, n, 4):
        s = slice(k, k + 4)
        re = re + ar[:, s] @ br[s]
        im = im + ai[:, s] @ br[s]
        if bi is not None:
            re = re + (-ai[:, s]) @ bi[s]
            im = im + ar[:, s] @ bi[s]
    return re, im


def dft2_dense(re, im=None, inverse=False):
    """The 2-D DFT as the dense products W x W of ir_op_dft2_f64 (the column transform first); returns (re, im)."""
    n = re.shape[0]
    c, s = twiddles(n)
    ws = s if inverse else -s
    tr, ti = _cgemm_k4(c, ws, np.asarray(re, np.float64), None if im is None else np.asarray(im, np.float64))
    yr, yi = _cgemm_k4(tr, ti, c, ws)
    if inverse:
        yr, yi = yr * (1.0 / (float(n) * n)), yi * (1.0 / (float(n) * n))
    return yr, yi


def dft2_scipy(re, im=None, inverse=False):
    import scipy.fft
    z = np.asarray(re, np.float64) if im is None else np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    y = scipy.fft.ifft2(z) if inverse else scipy.fft.fft2(z)
    return np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag)


# ---------------------------------------------------------------------------------------------------------------- step 3
def det_log(x: np.ndarray) -> np.ndarray:
    """log of positive normal doubles from IEEE additions, multiplications and one division in a stated order, so that every implementation gives
    the same bits: x = 2^k m with sqrt(2) / 2 <= m < sqrt(2), f = m - 1, s = f / (2 + f), z = s^2, w = z^2,
    R = z (L1 + w (L3 + w (L5 + w L7))) + w (L2 + w (L4 + w L6)), h = (0.5 f) f, log x = k ln2_hi - ((h - (s (h + R) + k ln2_lo)) - f): the
    reduction and the polynomial of fdlibm's e_log.c, always in its 0.5 f^2 form (below 1 ulp of error)."""
    lg = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01, 1.818357216161805012e-01,
          1.531383769920937332e-01, 1.479819860511658591e-01)
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    bits = np.ascontiguousarray(x, np.float64).view(np.uint64)
    hx = (bits >> np.uint64(32)).astype(np.int64)
    k = (hx >> 20) - 1023
    hx = hx & 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    hi = (hx | (i ^ 0x3ff00000)).astype(np.uint64)
    xm = ((hi << np.uint64(32)) | (bits & np.uint64(0xffffffff))).view(np.float64)
    k = k + (i >> 20)
    f = xm - 1.0
    s = f / (2.0 + f)
    dk = k.astype(np.float64)
    z = s * s
    w = z * z
    t1 = w * (lg[1] + w * (lg[3] + w * lg[5]))
    t2 = z * (lg[0] + w * (lg[2] + w * (lg[4] + w * lg[6])))
    r = t2 + t1
    h = (0.5 * f) * f
    return dk * ln2_hi - ((h - (s * (h + r) + dk * ln2_lo)) - f)


def mscn(y: np.ndarray) -> np.ndarray:
    k = gaussian_window(5, 5.0 / 6.0)
    h, w = y.shape
    yp = np.pad(y, 2, mode="edge")
    sq = yp * yp
    mu, m2 = np.zeros((h, w)), np.zeros((h, w))
    for i in range(5):
        for j in range(5):
            mu = mu + k[i, j] * yp[i:i + h, j:j + w]
            m2 = m2 + k[i, j] * sq[i:i + h, j:j + w]
    return (y - mu) / (np.sqrt(np.abs(m2 - mu * mu)) + 1.0)


def _conv_axis(x, taps, axis):
    """conv (kernel flipped) 'same' with zero padding along one axis, summed from 0.0 in tap order."""
    half = len(taps) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (half, half)
    xp = np.pad(x, pad)
    n = x.shape[axis]
    out = np.zeros_like(x)
    for t in range(len(taps)):   # tap t sits at offset t - half and multiplies x[. - (t - half)]
        start = 2 * half - t
        out = out + taps[t] * (xp[:, start:start + n] if axis == 1 else xp[start:start + n])
    return out


def derivatives(x, scale):
    """(Ix, Iy): conv2(x, dx / dy kernel, 'same') as two 11-tap passes, rows first."""
    xg, g = derivative_taps(scale)
    return _conv_axis(_conv_axis(x, xg, 1), g, 0), _conv_axis(_conv_axis(x, g, 1), xg, 0)


def downsample(x: np.ndarray) -> np.ndarray:
    k = gaussian_window(6, 0.9)
    h, w = x.shape
    xp = np.pad(x, ((2, 3), (2, 3)), mode="edge")
    out = np.zeros((h, w))
    for i in range(6):
        for j in range(6):
            out = out + k[i, j] * xp[i:i + h, j:j + w]
    return out[::2, ::2]


def planes_of_scale(o123, rgb, scale, dft="scipy", dft_fn=None):
    """[109][n][n] of step 3. dft: "scipy" or "dense"; dft_fn overrides both (the device call)."""
    fn = dft_fn or (dft2_dense if dft == "dense" else dft2_scipy)
    n = o123[0].shape[0]
    out = np.zeros((109, n, n))
    out[0] = mscn(o123[2])
    grads = [derivatives(o, scale) for o in o123]
    for c in range(3):
        ix, iy = grads[c]
        out[1 + c] = np.sqrt(ix * ix + iy * iy + EPS)
        out[7 + 2 * c], out[8 + 2 * c] = ix, iy
    logs = [det_log(c + K_LOG) for c in rgb]
    r, g, b = (v - wg_sum(v.reshape(-1), 1024) / float(v.size) for v in logs)
    out[4], out[5], out[6] = (r + g + b) / math.sqrt(3.0), (r + g - 2.0 * b) / math.sqrt(6.0), (r - g) / math.sqrt(2.0)
    fr, fi = fn(o123[2], None, False)
    bank = log_gabor_bank(n, scale)
    for f in range(12):
        re, im = fn(bank[f] * fr, bank[f] * fi, True)
        out[13 + 2 * f], out[14 + 2 * f] = re, im
        for part, p in enumerate((re, im)):
            dx, dy = derivatives(p, scale)
            out[37 + 4 * f + 2 * part], out[38 + 4 * f + 2 * part] = dx, dy
            out[85 + 2 * f + part] = np.sqrt(dx * dx + dy * dy) + EPS
    return out


def image_planes(img8, dft="scipy", dft_fn=None):
    """[(109, 504, 504), (109, 252, 252)]."""
    x = resize524(img8)
    rgb = [x[..., c] for c in range(3)]
    r, g, b = rgb
    o123 = [(0.3 * r + 0.04 * g) - 0.35 * b, (0.34 * r - 0.6 * g) + 0.17 * b, (0.06 * r + 0.63 * g) + 0.27 * b]
    p1 = planes_of_scale(o123, rgb, 1, dft, dft_fn)
    return [p1, planes_of_scale([downsample(v) for v in o123], [downsample(v) for v in rgb], 2, dft, dft_fn)]


# ---------------------------------------------------------------------------------------------------------------- step 4
def weibull_fit(x: np.ndarray, steps: bool = False):
    """Rows of positive values [rows][count] -> (k [rows], lambda [rows]) (and the Newton steps taken per row when asked)."""
    l = np.log(np.asarray(x, np.float64))
    mean = l.mean(axis=1)
    with np.errstate(all="ignore"):
        k = 1.2 / l.std(axis=1, ddof=1)
        live = np.ones(len(k), bool)
        taken = np.zeros(len(k), np.int64)
        for _ in range(WEIBULL_STEPS):
            if not live.any():
                break
            e = np.exp(k[live, None] * l[live])
            s0, s1, s2 = e.sum(axis=1), (e * l[live]).sum(axis=1), (e * (l[live] * l[live])).sum(axis=1)
            r = s1 / s0
            f, df = r - mean[live] - 1.0 / k[live], s2 / s0 - r * r + 1.0 / (k[live] * k[live])
            kn = k[live] - f / df
            done = np.abs(kn - k[live]) < WEIBULL_TOL
            k[live] = kn
            taken[live] += 1
            live[np.flatnonzero(live)[done]] = False
        lam = np.exp(k[:, None] * l).mean(axis=1) ** (1.0 / k)
    return (k, lam, taken) if steps else (k, lam)


def _blocks(p, b):
    """[n][n] -> [36][b * b], blocks row-major."""
    g = p.shape[0] // b
    return p.reshape(g, b, g, b).transpose(0, 2, 1, 3).reshape(g * g, b * b)


def wg_sum(v: np.ndarray, threads: int = 256) -> np.ndarray:
    """The sum over the last axis in the ONE order the definition fixes for a block's sums (and the kernels use): partial t of 256 adds elements
    t, t + 256, ... from 0.0; the partials fold in groups of 64 by xor 32, 16, 8, 4, 2, 1; the groups are added in turn. (threads = 1024: the
    order of a whole plane's sum.)"""
    count = v.shape[-1]
    rows = -(-count // threads)
    p = np.zeros(v.shape[:-1] + (rows * threads,))
    p[..., :count] = v
    p = p.reshape(v.shape[:-1] + (rows, threads))
    acc = np.zeros(v.shape[:-1] + (threads,))
    for r in range(rows):
        acc = acc + p[..., r, :]
    acc = acc.reshape(v.shape[:-1] + (threads // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    total = acc[..., 0, 0]
    for g in range(1, threads // 64):
        total = total + acc[..., g, 0]
    return total


def _six(v):
    """[..., count] -> [..., 6]."""
    neg, pos, sq = v < 0, v > 0, v * v
    return np.stack([neg.sum(-1).astype(np.float64), pos.sum(-1).astype(np.float64), wg_sum(np.where(neg, sq, 0.0)), wg_sum(np.where(pos, sq, 0.0)),
                     wg_sum(np.abs(v)), wg_sum(sq)], -1)


def scale_stats(planes: np.ndarray, scale: int, weibull=None) -> np.ndarray:
    """[109][n][n] -> [36][558]."""
    b = BLOCK // scale
    out = np.zeros((36, STATS))
    m = _blocks(planes[0], b).reshape(36, b, b)
    fields = [m] + [m * np.roll(m, s, axis=(1, 2)) for s in SHIFTS]
    out[:, :30] = np.stack([_six(f.reshape(36, -1)) for f in fields], 1).reshape(36, 30)
    for p in range(78):
        out[:, 30 + 6 * p:36 + 6 * p] = _six(_blocks(planes[7 + p], b))
    for p in range(3):
        v = _blocks(planes[4 + p], b)
        mean = wg_sum(v) / float(b * b)
        out[:, 498 + 2 * p] = mean
        d = v - mean[:, None]
        out[:, 499 + 2 * p] = wg_sum(d * d) / float(b * b - 1)
    mags = np.concatenate([_blocks(planes[p], b) for p in (1, 2, 3) + tuple(range(85, 109))])   # [27 * 36][b b], plane-major
    k, lam = (weibull or weibull_fit)(mags)
    out[:, 504:558:2] = k.reshape(27, 36).T
    out[:, 505:558:2] = lam.reshape(27, 36).T
    return out


def image_stats(img8, dft="scipy", dft_fn=None, weibull=None) -> np.ndarray:
    """Steps 1-4 up to the fits: [2][36][558]."""
    p = image_planes(img8, dft, dft_fn)
    return np.stack([scale_stats(p[0], 1, weibull), scale_stats(p[1], 2, weibull)])


_gam = None


def gam_table():
    global _gam
    if _gam is None:
        gam = np.arange(0.2, 10.001, 0.001)
        _gam = (gam, np.array([math.exp(2.0 * math.lgamma(2.0 / g) - math.lgamma(1.0 / g) - math.lgamma(3.0 / g)) for g in gam]))
    return _gam


_lg = np.frompyfunc(math.lgamma, 1, 1)


def aggd_from_six(six: np.ndarray, count: int):
    """[..., 6] -> (alpha, beta_l, beta_r, mean): NIQE's fit; the first minimum of |r_gam - rn| wins, a NaN rn takes entry 0."""
    gam, r_gam = gam_table()
    cl, cr, sl, sr, sa, ss = (six[..., k] for k in range(6))
    with np.errstate(all="ignore"):
        ls, rs = np.sqrt(sl / cl), np.sqrt(sr / cr)
        g = ls / rs
        rhat = (sa / count) ** 2 / (ss / count)
        rn = rhat * (g ** 3 + 1.0) * (g + 1.0) / (g ** 2 + 1.0) ** 2
        safe = np.where(np.isfinite(rn), rn, -np.inf)
        hi = np.clip(np.searchsorted(r_gam, safe, side="left"), 0, len(gam) - 1)
        lo = np.clip(hi - 1, 0, len(gam) - 1)
        alpha = gam[np.where(np.abs(r_gam[lo] - safe) <= np.abs(r_gam[hi] - safe), lo, hi)]
        lg1, lg2, lg3 = (_lg(v / alpha).astype(np.float64) for v in (1.0, 2.0, 3.0))
        sc = np.sqrt(np.exp(lg1 - lg3))
        bl, br = ls * sc, rs * sc
        return alpha, bl, br, (br - bl) * np.exp(lg2 - lg1)


def features_from_stats(stats: np.ndarray) -> np.ndarray:
    """[2][36][558] -> [36][468]."""
    feat = np.zeros((36, FEATURES))
    for s in range(2):
        count = (BLOCK // (s + 1)) ** 2
        st = stats[s]
        a, bl, br, mean = aggd_from_six(st[:, :30].reshape(36, 5, 6), count)
        cols = [a[:, 0], (bl[:, 0] + br[:, 0]) / 2.0]
        for f in range(1, 5):
            cols += [a[:, f], mean[:, f], bl[:, f], br[:, f]]
        wb = st[:, 504:558].reshape(36, 27, 2)
        for p in range(3):
            cols += [wb[:, p, 1], wb[:, p, 0]]           # (scale, shape) = (lambda, k)
        cols += [st[:, 498 + i] for i in range(6)]
        a, bl, br, _ = aggd_from_six(st[:, 30:498].reshape(36, 78, 6), count)
        for p in range(78):
            cols += [a[:, p], (bl[:, p] + br[:, p]) / 2.0]
        for p in range(3, 27):
            cols += [wb[:, p, 1], wb[:, p, 0]]
        feat[:, 234 * s:234 * s + 234] = np.stack(cols, 1)
    return feat


# ---------------------------------------------------------------------------------------------------------------- step 5
def score_features(feat: np.ndarray, params) -> float:
    mu_p, cov_p, mean_s, pv = params
    feat = np.asarray(feat, np.float64)
    with np.errstate(invalid="ignore"):
        feat = np.where(feat > INF_CONST, INF_CONST, feat)
    c = (feat - mean_s.reshape(1, -1)) @ pv
    nan = np.isnan(c)
    ok = ~nan.any(axis=1)
    if int(ok.sum()) < 2:
        raise ValueError("IL-NIQE needs two feature rows without NaN")
    with np.errstate(all="ignore"):
        mu_d = np.where(nan, 0.0, c).sum(axis=0) / (~nan).sum(axis=0)
    c = np.where(nan, mu_d[None, :], c)
    rows = c[ok]
    cen = rows - rows.mean(axis=0)
    cov_d = cen.T @ cen / (rows.shape[0] - 1)
    inv = np.linalg.pinv((np.asarray(cov_p, np.float64) + cov_d) / 2.0)
    d = c - np.asarray(mu_p, np.float64).reshape(1, -1)
    return float(np.mean(np.sqrt(np.einsum("bi,ij,bj->b", d, inv, d))))


def ilniqe(img8, params, **kw) -> float:
    return score_features(features_from_stats(image_stats(img8, **kw)), params)


def load_params(path):
    """(mu_prisparam [d], cov_prisparam [d][d], meanOfSampleData [468], principleVectors [468][d]) of a .mat or an .npz."""
    names = ("mu_prisparam", "cov_prisparam", "meanOfSampleData", "principleVectors")
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            if any(k not in z.files for k in names):
                raise ValueError(f"{path}: {', '.join(k for k in names if k not in z.files)} missing")
            got = [np.asarray(z[k], np.float64) for k in names]
    else:
        from scipy.io import loadmat
        m = loadmat(str(path))
        if "templateModel" not in m or m["templateModel"].size != 4:
            raise ValueError(f"{path}: no 1 x 4 cell templateModel")
        got = [np.asarray(v, np.float64) for v in m["templateModel"].reshape(-1)]
    mu, cov, mean_s, pv = got
    mu, mean_s = mu.reshape(-1), mean_s.reshape(-1)
    d = mu.size
    if d < 1 or cov.shape != (d, d) or mean_s.shape != (FEATURES,) or pv.shape != (FEATURES, d):
        raise ValueError(f"{path}: mu_prisparam {mu.shape}, cov_prisparam {cov.shape}, meanOfSampleData {mean_s.shape}, principleVectors {pv.shape} "
                         f"are not [d], [d][d], [468], [468][d]")
    if not all(np.isfinite(v).all() for v in (mu, cov, mean_s, pv)):
        raise ValueError(f"{path}: the template holds NaN or infinity")
    return mu, cov, mean_s, pv


def evaluate(img_dir, params, ntest=None, backend="host", log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    par = load_params(params)
    ctx = iq = None
    if backend == "gpu":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from instarevive_amd import _lib as L, ilniqe as iq
        ctx = L.Context(0)
        iq.configure(ctx)
    total, scored, skipped = 0.0, 0, 0
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            v = iq.score_arrays(ctx, img, par) if ctx is not None else ilniqe(img, par)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"ilniqe: {total / scored:.5f}")
    return total / scored if scored else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--ilniqe_params", required=True, help="ILNIQE_templateModel.mat or an .npz with mu_prisparam / cov_prisparam / meanOfSampleData / principleVectors")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    evaluate(a.img_path, a.ilniqe_params, a.ntest, backend=a.backend)


if __name__ == "__main__":
    main()
