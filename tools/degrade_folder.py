#!/usr/bin/env python
"""Synthesise the low-quality inputs of a restoration run from ground truth: the definition (numpy) and a folder tool.

The reference makes its LQ sets with tools/lq.py (blur()), the first-order chain of dataset/codeformer.py:CodeformerDataset.__getitem__
(:140-163): a K x K Gaussian blur (cv2.filter2D), a bilinear downsample by U[2,4], Gaussian noise, a JPEG round trip, a bilinear resize back.
This file restates that chain without OpenCV, down to the order of operations, and is the model of ir_degrade (csrc/degrade.hip), which
equals it byte for byte. For one RGB8 image h x w (`degrade_model`):

  1. x = float32(v / 255.0), the division in double.
  2. blur: correlation with a K x K float64 kernel (K odd), border BORDER_REFLECT_101, every channel accumulated in float64 in row-major tap
     order with separate multiplies and adds (acc += k[t] * shifted), rounded once to float32. cv2.filter2D takes a DFT path for a kernel
     this large, so parity with it holds to rounding only (docs/parity.md). min(h, w) < K // 2 + 1 is refused.
  3. bilinear to lh x lw (cv2.resize INTER_LINEAR on floats, no antialiasing): fx = float32((dx + 0.5) * (w / lw) - 0.5) with the product in
     double, sx = floor(fx), fx -= sx; sx < 0 -> (0, 0); sx >= w - 1 -> (w - 1, 0); a0 S[sx] + a1 S[sx + 1] along the rows, then the same
     form down the columns, float32 with two multiplies and one add each.
  4. noise: x += float32(n) * float32(sigma) / 255 in float32 (utils/degradation.py:435), clip to [0, 1]; n is a float32 standard-normal
     field [lh][lw][3]. None skips the step.
  5. JPEG round trip at quality q in 1 .. 100 of the bytes rint(x * 255) (half to even, cv2.imencode's conversion): libjpeg's pixel
     pipeline in integers (`jpeg_roundtrip`; baseline, 4:2:0, ISLOW DCT, fancy upsampling - Pillow's and OpenCV's defaults), then
     float32(byte) / 255. Entropy coding is lossless, so no Huffman coder is needed. q = 0 skips the step.
  6. bilinear back to h x w, the function of step 3.
  7. norm "none": uint8(trunc(clip(x, 0, 1) * 255)); norm "max": uint8(trunc(max(x, 0) / m * 255)) with m the maximum of the step-6 image
     over all pixels and channels - tools/lq.py:45 literally, its brightening included (an all-black image, m = 0, stays black).

The folder tool draws every file's parameters as the command lines do (instarevive_amd/degrade.py: seeded by --degrade_seed and the file's
relative path) and writes the LQ images as PNG; --backend gpu takes the pixels from ir_degrade instead of the model.

`--degrade realesrgan` is the reference's SECOND-ORDER recipe (configs/general_deg_realesrgan_val.yaml): its definition is `degrade_chain_model`
below, a per-image list of ops, which ir_degrade_chain (csrc/degrade_chain.hip) equals in bytes and in every intermediate float.
"""
import argparse
import math
import os
import sys
from pathlib import Path

import numpy as np

ROOT = str(Path(__file__).resolve().parent.parent)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NORM_NONE, NORM_MAX = 0, 1
MIN_LOW = 8   # ir_degrade's bound on lh and lw (libjpeg replicates chroma instead of interpolating it when the chroma plane is <= 2 wide)

# ---------------------------------------------------------------- steps 1 - 4, 6, 7


def to_float(img8: np.ndarray) -> np.ndarray:
    return (img8.astype(np.float64) / 255.0).astype(np.float32)


def blur(x: np.ndarray, k: np.ndarray) -> np.ndarray:
    """Step 2 on float32 [h][w][c]."""
    k = np.asarray(k, dtype=np.float64)
    K = k.shape[0]
    if k.shape != (K, K) or K % 2 == 0:
        raise ValueError("the blur kernel must be K x K with K odd")
    R = K // 2
    h, w = x.shape[:2]
    if min(h, w) < R + 1:
        raise ValueError(f"a {h} x {w} image is too small for a {K} x {K} blur (reflection needs {R + 1} pixels)")
    p = np.pad(x.astype(np.float64), ((R, R), (R, R), (0, 0)), mode="reflect")   # reflect = BORDER_REFLECT_101
    acc = np.zeros(x.shape, dtype=np.float64)
    for a in range(K):
        for b in range(K):
            acc += k[a, b] * p[a:a + h, b:b + w]
    return acc.astype(np.float32)


def _axis_table(src: int, dst: int):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (src / dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s[lo], f[lo] = 0, 0.0
    s[hi], f[hi] = src - 1, 0.0
    return s, np.minimum(s + 1, src - 1), (np.float32(1.0) - f).astype(np.float32), f


def bilinear(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """Steps 3 and 6 on float32 [h][w][c]."""
    h, w = x.shape[:2]
    x0, x1, a0, a1 = _axis_table(w, ow)
    y0, y1, b0, b1 = _axis_table(h, oh)
    rows = a0[None, :, None] * x[:, x0] + a1[None, :, None] * x[:, x1]
    assert rows.dtype == np.float32
    return b0[:, None, None] * rows[y0] + b1[:, None, None] * rows[y1]


def add_noise(x: np.ndarray, n: np.ndarray, sigma) -> np.ndarray:
    noise = np.asarray(n, dtype=np.float32) * np.float32(sigma) / np.float32(255.0)
    return np.clip(x + noise, np.float32(0.0), np.float32(1.0))


def to_bytes(x: np.ndarray, norm: int = NORM_NONE) -> np.ndarray:
    if norm == NORM_MAX:
        m = x.max()
        if not m > 0:
            return np.zeros(x.shape, dtype=np.uint8)
        return (np.maximum(x, np.float32(0.0)) / m * np.float32(255.0)).astype(np.uint8)
    return (np.clip(x, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)


# ---------------------------------------------------------------- step 5: libjpeg's pixel pipeline

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                    + [99] * 32, dtype=np.int64).reshape(8, 8)
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def quant_tables(q: int):
    """The two tables of jpeg_set_quality(q, force_baseline), natural order."""
    if not 1 <= q <= 100:
        raise ValueError("JPEG quality must be 1 .. 100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q))


def _fix(x):
    return int(x * 65536 + 0.5)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first: bool):
    """jfdctint.c over the last axis of int64 [...][8]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 + t12 * (-F_1_847), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961), z4 * (-F_0_390)
    z3, z4 = z3 + z5, z4 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _idct_pass(c, first: bool):
    """jidctint.c over the last axis of int64 [...][8]."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (c[..., i] for i in range(8))
    z1 = (i2 + i6) * F_0_541
    t2, t3 = z1 + i6 * (-F_1_847), z1 + i2 * F_0_765
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = z1 * (-F_0_899), z2 * (-F_2_562), z3 * (-F_1_961), z4 * (-F_0_390)
    z3, z4 = z3 + z5, z4 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 13 - 2 if first else 13 + 2 + 3
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def dct_roundtrip(plane: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """Forward DCT, quantise, dequantise, inverse DCT of every 8 x 8 block of a uint8 plane whose sides are multiples of 8."""
    H, W = plane.shape
    b = plane.astype(np.int64).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3) - 128   # [by][bx][row][col]
    c = _fdct_pass(b, True)                                               # along the rows
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)            # down the columns; the result is scaled by 8
    q = np.sign(c) * ((np.abs(c) + 4 * qt) // (8 * qt)) * qt              # quantise with rounding, dequantise
    s = _idct_pass(q.swapaxes(-1, -2), True).swapaxes(-1, -2)             # down the columns
    s = _idct_pass(s, False)                                              # along the rows
    out = np.clip(s + 128, 0, 255).astype(np.uint8)
    return out.transpose(0, 2, 1, 3).reshape(H, W)


def _pad_edge(a: np.ndarray, H: int, W: int) -> np.ndarray:
    return np.pad(a, ((0, H - a.shape[0]), (0, W - a.shape[1])), mode="edge")


def jpeg_roundtrip(rgb: np.ndarray, q: int) -> np.ndarray:
    """The pixels libjpeg decodes from what it encodes of uint8 [h][w][3] at quality q: Image.save(format="JPEG", quality=q) then Image.open."""
    h, w = rgb.shape[:2]
    ql, qc = quant_tables(q)
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    PH, PW = (h + 15) & ~15, (w + 15) & ~15
    ch, cw = (h + 1) // 2, (w + 1) // 2
    planes = [dct_roundtrip(_pad_edge(y, PH, PW).astype(np.uint8), ql)[:h, :w].astype(np.int64)]
    bias = np.tile(np.array([1, 2], dtype=np.int64), PW // 4)
    for c in (cb, cr):
        f = _pad_edge(c, 2 * ch, PW)   # columns to a multiple of 16, rows only to an even count
        d = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2] + bias) >> 2
        d = _pad_edge(d, PH // 2, PW // 2)   # then the last downsampled row out to a multiple of 8
        planes.append(dct_roundtrip(d.astype(np.uint8), qc)[:ch, :cw].astype(np.int64))
    up = []
    for c in planes[1:]:   # h2v2_fancy_upsample on the true chroma size
        above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
        cs = np.empty((2 * ch, cw), dtype=np.int64)
        cs[0::2], cs[1::2] = 3 * c + above, 3 * c + below
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1), np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        o = np.empty((2 * ch, 2 * cw), dtype=np.int64)
        o[:, 0::2], o[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4   # at the ends left / right is cs itself: (4 cs + 8 or 7) >> 4
        up.append(o[:h, :w] - 128)
    yy, cbp, crp = planes[0], up[0], up[1]
    out = np.stack([yy + ((_fix(1.402) * crp + 32768) >> 16),
                    yy + ((-_fix(.34414) * cbp - _fix(.71414) * crp + 32768) >> 16),
                    yy + ((_fix(1.772) * cbp + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def jpeg_step(x: np.ndarray, q: int):
    """Step 5 on float32 [lh][lw][3] in [0, 1] -> (float32 image, the decoded bytes)."""
    b = jpeg_roundtrip(np.clip(np.rint(x * np.float32(255.0)), 0, 255).astype(np.uint8), q)   # saturate_cast
    return b.astype(np.float32) / np.float32(255.0), b


# ---------------------------------------------------------------- the chain


def degrade_model(img8: np.ndarray, kernel: np.ndarray, lh: int, lw: int, sigma: float = 0.0, q: int = 0, noise=None, norm: int = NORM_NONE,
                  with_jpeg: bool = False):
    """The LQ image (uint8 [h][w][3]) of a ground-truth image; with_jpeg: also the lh x lw bytes behind the JPEG step (None for q = 0)."""
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise ValueError("the image must be HWC uint8 RGB")
    h, w = img8.shape[:2]
    if not (1 <= lh <= h and 1 <= lw <= w):
        raise ValueError("the low-resolution size must lie inside the image's")
    x = blur(to_float(img8), kernel)
    x = bilinear(x, lh, lw)
    if noise is not None:
        x = add_noise(x, noise, sigma)
    mid = None
    if q:
        x, mid = jpeg_step(x, q)
    out = to_bytes(bilinear(x, h, w), norm)
    return (out, mid) if with_jpeg else out


# ---------------------------------------------------------------- the second-order chain (ir_degrade_chain, csrc/degrade_chain.hip)
# The reference validates general super-resolution with the Real-ESRGAN recipe (configs/general_deg_realesrgan_val.yaml, dataset/realesrgan.py,
# dataset/batch_transform.py:RealESRGANBatchTransform): blur, resize, noise, DiffJPEG, then a second such stage, a final sinc filter and a
# bicubic resize back. Here that is a CHAIN: per image a list of at most CHAIN_MAX_OPS ops on a float32 [h][w][3] image that starts as
# to_float(img8), and the bytes uint8(clip(rint(x * 255), 0, 255)) behind the last one (`finish`; torch.round rounds half to even). The ops:
#   (OP_FILTER, kernel)                 utils/image/common.py:filter2D = blur() above with a K x K float64 kernel, K odd and at most 21.
#   (OP_RESIZE, mode, oh, ow, scale)    F.interpolate without antialiasing. scale = 0: the call passed size=(oh, ow) and the source coordinate
#                                       uses float32(in) / float32(out); scale > 0: the call passed scale_factor=scale, oh = floor(in * scale)
#                                       in double, and the coordinate uses float32(1 / scale) - torch's rule, not in / out. The coordinate
#                                       is float32(s * (d + 0.5) - 0.5), fused as torch's CPU kernels are (_src_coord); bilinear clamps a negative
#                                       coordinate to 0, bicubic (A = -0.75, weights in float32) clamps its four indices to the image instead;
#                                       area is adaptive_avg_pool2d's window floor(o * in / out) .. ceil((o + 1) * in / out), also when the
#                                       output is larger. The taps (4, 16, the window) are summed in fp64 in row-major order as
#                                       acc += (wy * wx) * x - area: acc += x, then acc / count - and rounded once.
#   (OP_GAUSS, field, sigma, gray)      add_noise() above; gray: one [h][w] field for the three channels.
#   (OP_POISSON, u, scale, gray)        utils/degradation.py:generate_poisson_noise_pt with the Poisson draw made by inversion from the uniform
#                                       field u (float64, [h][w][3], gray: [h][w]): see poisson_noise().
#   (OP_DIFFJPEG, quality)              the clamp to [0, 1] that precedes every call, then utils/image/diffjpeg.py:DiffJPEG(differentiable=False)
#                                       at a float32 quality: see diffjpeg().
OP_FILTER, OP_RESIZE, OP_GAUSS, OP_POISSON, OP_DIFFJPEG = 1, 2, 3, 4, 5
MODE_AREA, MODE_BILINEAR, MODE_BICUBIC = 0, 1, 2
CHAIN_MAX_OPS, CHAIN_MAX_KSIZE, POISSON_MAX_K = 16, 21, 1024
_F = np.float32


def _src_scale(src: int, dst: int, scale: float):
    return _F(1.0 / scale) if scale else _F(src) / _F(dst)


def _src_coord(src: int, dst: int, scale: float) -> np.ndarray:
    """float32(s * (d + 0.5) - 0.5) with d + 0.5 in float32 and the product and the difference in double: torch's CPU kernels are compiled
    to a fused multiply-add here (measured: with a separate float32 multiply the bilinear resize is 2e-6 away from torch, with this 1.2e-7)."""
    d = (np.arange(dst, dtype=np.float32) + _F(0.5)).astype(np.float64)
    return (np.float64(_src_scale(src, dst, scale)) * d - 0.5).astype(np.float32)


def _linear_taps(src: int, dst: int, scale: float):
    real = np.maximum(_src_coord(src, dst, scale), _F(0.0))
    i0 = np.minimum(real.astype(np.int64), src - 1)
    lam = np.clip(real - i0.astype(np.float32), _F(0.0), _F(1.0))
    return [i0, i0 + (i0 < src - 1)], [_F(1.0) - lam, lam]


def _cubic_taps(src: int, dst: int, scale: float):
    real = _src_coord(src, dst, scale)
    fl = np.floor(real)
    t = np.clip(real - fl, _F(0.0), _F(1.0))
    i = fl.astype(np.int64)
    a = _F(-0.75)

    def near(x):   # |x| <= 1
        return ((a + _F(2.0)) * x - (a + _F(3.0))) * x * x + _F(1.0)

    def far(x):    # 1 < |x| < 2
        return ((a * x - _F(5.0) * a) * x + _F(8.0) * a) * x - _F(4.0) * a
    u = _F(1.0) - t
    wts = [far(t + _F(1.0)), near(t), near(u), far(u + _F(1.0))]
    assert all(v.dtype == np.float32 for v in wts)
    return [np.clip(i + k, 0, src - 1) for k in (-1, 0, 1, 2)], wts


def _area(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    h, w = x.shape[:2]
    o = np.arange(oh, dtype=np.int64)
    y0, y1 = (o * h) // oh, ((o + 1) * h + oh - 1) // oh
    o = np.arange(ow, dtype=np.int64)
    x0, x1 = (o * w) // ow, ((o + 1) * w + ow - 1) // ow
    xd = x.astype(np.float64)
    acc = np.zeros((oh, ow, x.shape[2]), dtype=np.float64)
    for a in range(int((y1 - y0).max())):
        for b in range(int((x1 - x0).max())):
            live = ((y0 + a < y1)[:, None] & (x0 + b < x1)[None, :])[..., None]
            acc += np.where(live, xd[np.minimum(y0 + a, h - 1)][:, np.minimum(x0 + b, w - 1)], 0.0)   # + 0.0 leaves an fp64 sum as it is
    return (acc / ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(np.float64)[..., None]).astype(np.float32)


def resize(x: np.ndarray, mode: int, oh: int, ow: int, scale: float = 0.0) -> np.ndarray:
    """OP_RESIZE on float32 [h][w][c]."""
    h, w = x.shape[:2]
    if scale and (oh, ow) != (int(math.floor(h * scale)), int(math.floor(w * scale))):
        raise ValueError("with a scale factor the output size is floor(in * scale)")
    if oh < 1 or ow < 1 or mode not in (MODE_AREA, MODE_BILINEAR, MODE_BICUBIC):
        raise ValueError("resize: an empty output or an unknown mode")
    if mode == MODE_AREA:
        return _area(x, oh, ow)
    taps = _linear_taps if mode == MODE_BILINEAR else _cubic_taps
    (yi, yw), (xi, xw) = taps(h, oh, scale), taps(w, ow, scale)
    xd = x.astype(np.float64)
    acc = np.zeros((oh, ow, x.shape[2]), dtype=np.float64)
    for iy, wy in zip(yi, yw):
        for ix, wx in zip(xi, xw):
            acc += (wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :])[..., None] * xd[iy][:, ix]
    return acc.astype(np.float32)


def levels_of(x: np.ndarray) -> np.ndarray:
    """clip(rint(x * 255), 0, 255) of a float32 array, as integers: the level r = level / 255 of the Poisson rate."""
    return np.clip(np.rint(x * _F(255.0)), 0, 255).astype(np.int64)


def poisson_vals(levels: np.ndarray) -> int:
    """2 ** ceil(log2(number of distinct levels)): 1, 2, 4 .. 256."""
    n, v = len(np.unique(levels)), 1
    while v < n:
        v *= 2
    return v


def poisson_exp_table() -> np.ndarray:
    """exp(-lambda) for the 9 values of vals and the 256 levels, float64 [9][256]: an INPUT of the device call, so that no difference between
    two libms can enter the bytes."""
    r = np.arange(256, dtype=np.float32) / _F(255.0)
    return np.stack([np.exp(-(r * _F(1 << j)).astype(np.float64)) for j in range(9)])


def poisson_invert(lam: np.ndarray, p0: np.ndarray, u: np.ndarray) -> np.ndarray:
    """The smallest k whose cumulative sum p(0) + .. + p(k) exceeds u, p(k + 1) = p(k) * lam / (k + 1) in fp64 with separate operations
    (at most POISSON_MAX_K: a u above every sum fp64 can reach stops there)."""
    lam, u = np.asarray(lam, dtype=np.float64), np.asarray(u, dtype=np.float64)
    p = np.array(p0, dtype=np.float64)
    cum, k = p.copy(), np.zeros(p.shape, dtype=np.int64)
    live = np.nonzero(cum <= u)
    for it in range(1, POISSON_MAX_K + 1):
        if live[0].size == 0:
            break
        p[live] = p[live] * lam[live] / float(it)
        cum[live] = cum[live] + p[live]
        k[live] = it
        keep = cum[live] <= u[live]
        live = tuple(ix[keep] for ix in live)
    return k


def poisson_noise(x: np.ndarray, u: np.ndarray, scale, gray: bool, table=None) -> np.ndarray:
    """OP_POISSON. gray: the levels are those of float32 (0.2989 R + 0.587 G) + 0.114 B (torchvision's rgb_to_grayscale) and one noise value
    goes to the three channels. r = level / 255, vals from the count of distinct levels, lambda = r * vals, P by inversion, the noise
    (P / vals - r) * scale in float32 is added to the unrounded x and the sum clipped to [0, 1]."""
    table = poisson_exp_table() if table is None else table
    base = (_F(0.2989) * x[..., 0] + _F(0.587) * x[..., 1]) + _F(0.114) * x[..., 2] if gray else x
    if u.shape != base.shape:
        raise ValueError("the uniform field must be [h][w] for gray noise and [h][w][3] otherwise")
    lv = levels_of(base)
    vals = poisson_vals(lv)
    r = lv.astype(np.float32) / _F(255.0)
    lam = r * _F(vals)
    k = poisson_invert(lam, table[vals.bit_length() - 1][lv], u)
    noise = (k.astype(np.float32) / _F(vals) - r) * _F(scale)
    assert noise.dtype == np.float32
    return np.clip(x + (noise[..., None] if gray else noise), _F(0.0), _F(1.0))


def gauss_noise(x: np.ndarray, field: np.ndarray, sigma, gray: bool) -> np.ndarray:
    """OP_GAUSS."""
    if field.shape != (x.shape[:2] if gray else x.shape):
        raise ValueError("the normal field must be [h][w] for gray noise and [h][w][3] otherwise")
    return add_noise(x, field[..., None] if gray else field, sigma)


# DiffJPEG: the module's tables are the TRANSPOSES of libjpeg's, its colour matrices and its cosine basis are float32
JPEG_TABLES = (LUMA_Q.T.astype(np.float32), CHROMA_Q.T.astype(np.float32))
RGB_TO_YCC = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=np.float32)   # [out][in]
YCC_SHIFT = np.array([0.0, 128.0, 128.0], dtype=np.float32)
YCC_TO_RGB = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=np.float32)   # [out][in]
_ALPHA = np.array([1.0 / np.sqrt(2)] + [1.0] * 7)
DCT_SCALE = (np.outer(_ALPHA, _ALPHA) * 0.25).astype(np.float32).reshape(64)
IDCT_ALPHA = np.outer(_ALPHA, _ALPHA).astype(np.float32).reshape(64)


def dct_basis() -> np.ndarray:
    """float64 [64][64] holding the module's float32 basis: [8 x + y][8 u + v] = float32(cos((2 x + 1) u pi / 16) cos((2 y + 1) v pi / 16)),
    sample (x, y), frequency (u, v). The inverse transform's tensor is its transpose. An INPUT of the device call, like the blur kernel."""
    i = np.arange(8)
    c = np.cos((2 * i[:, None] + 1) * i[None, :] * np.pi / 16)   # [sample][frequency]
    return (c[:, None, :, None] * c[None, :, None, :]).astype(np.float32).astype(np.float64).reshape(64, 64)


def jpeg_factor(quality) -> np.float32:
    """quality_to_factor on a float32 tensor element, as the batch transform passes one."""
    q = _F(quality)
    return (_F(5000.0) / q if q < 50 else _F(200.0) - q * _F(2.0)) / _F(100.0)


def _blocks(p: np.ndarray) -> np.ndarray:
    H, W = p.shape
    return p.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


def _unblocks(b: np.ndarray, H: int, W: int) -> np.ndarray:
    return b.reshape(H // 8, W // 8, 8, 8).transpose(0, 2, 1, 3).reshape(H, W)


def jpeg_planes(x: np.ndarray):
    """float32 [h][w][3] in [0, 1] -> the Y plane [H][W] and the Cb and Cr planes [H / 2][W / 2] (H, W: h, w up to multiples of 16, zero padded
    BEFORE the colour matrix). Every 3-term sum is fp64, ((m0 r + m1 g) + m2 b) + shift, rounded once; the 2 x 2 mean is ((a + b) + c + d) / 4."""
    h, w = x.shape[:2]
    H, W = (h + 15) & ~15, (w + 15) & ~15
    p = np.zeros((H, W, 3), dtype=np.float32)
    p[:h, :w] = x
    v = (p * _F(255.0)).astype(np.float64)
    m = RGB_TO_YCC.astype(np.float64)
    ycc = [(((m[c, 0] * v[..., 0] + m[c, 1] * v[..., 1]) + m[c, 2] * v[..., 2]) + float(YCC_SHIFT[c])).astype(np.float32) for c in range(3)]
    out = [ycc[0]]
    for c in ycc[1:]:
        d = c.astype(np.float64)
        out.append(((((d[0::2, 0::2] + d[0::2, 1::2]) + d[1::2, 0::2]) + d[1::2, 1::2]) / 4.0).astype(np.float32))
    return out


def jpeg_quotients(plane: np.ndarray, table: np.ndarray, factor, basis: np.ndarray) -> np.ndarray:
    """The forward DCT of every 8 x 8 block of a float32 plane over table * factor, before the rounding: float32 [blocks][64]. The 64-term
    sum over the samples is fp64 in row-major order, scaled and rounded once; table * factor and the division are float32 operations."""
    d = _blocks(plane).astype(np.float64) - 128.0
    acc = np.zeros(d.shape, dtype=np.float64)
    for s in range(64):
        acc += d[:, s:s + 1] * basis[s][None, :]
    coef = (DCT_SCALE.astype(np.float64)[None, :] * acc).astype(np.float32)
    return coef / (table.reshape(64) * _F(factor))[None, :]


def jpeg_plane_back(coef: np.ndarray, table: np.ndarray, factor, basis: np.ndarray, H: int, W: int) -> np.ndarray:
    """Integer coefficients [blocks][64] -> the float32 plane: times table * factor, times alpha (float32), the 64-term sum over the
    frequencies in fp64 in row-major order, float32(0.25 * sum + 128)."""
    e = ((coef.astype(np.float32) * (table.reshape(64) * _F(factor))[None, :]) * IDCT_ALPHA[None, :]).astype(np.float64)
    acc = np.zeros(e.shape, dtype=np.float64)
    for f in range(64):
        acc += e[:, f:f + 1] * basis[:, f][None, :]
    return _unblocks((0.25 * acc + 128.0).astype(np.float32), H, W)


def jpeg_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, h: int, w: int) -> np.ndarray:
    """Replicated chroma, (Cb, Cr) - 128 in float32, the inverse matrix as an fp64 3-term sum rounded once, the clamp to [0, 255], / 255, the crop."""
    planes = [y.astype(np.float64)] + [(np.repeat(np.repeat(c, 2, axis=0), 2, axis=1) - _F(128.0)).astype(np.float64) for c in (cb, cr)]
    m = YCC_TO_RGB.astype(np.float64)
    rgb = np.stack([((m[c, 0] * planes[0] + m[c, 1] * planes[1]) + m[c, 2] * planes[2]).astype(np.float32) for c in range(3)], axis=-1)
    return (np.clip(rgb, _F(0.0), _F(255.0)) / _F(255.0))[:h, :w]


def diffjpeg(x: np.ndarray, quality, basis=None) -> np.ndarray:
    """OP_DIFFJPEG on float32 [h][w][3]."""
    basis = dct_basis() if basis is None else basis
    h, w = x.shape[:2]
    H, W = (h + 15) & ~15, (w + 15) & ~15
    f = jpeg_factor(quality)
    planes = jpeg_planes(np.clip(x, _F(0.0), _F(1.0)))
    back = []
    for i, p in enumerate(planes):
        t = JPEG_TABLES[min(i, 1)]
        back.append(jpeg_plane_back(np.rint(jpeg_quotients(p, t, f, basis)), t, f, basis, *p.shape))
    return jpeg_rgb(back[0], back[1], back[2], h, w)


def finish(x: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(x * _F(255.0)), 0, 255).astype(np.uint8)


def degrade_chain_model(img8: np.ndarray, ops, tap=None, table=None, basis=None):
    """The LQ bytes of a ground-truth image under a chain (the size behind the last op is the LQ image's); with `tap` = an op's index also
    the float32 image behind that op."""
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise ValueError("the image must be HWC uint8 RGB")
    if len(ops) > CHAIN_MAX_OPS:
        raise ValueError(f"a chain holds at most {CHAIN_MAX_OPS} ops")
    x, kept = to_float(img8), None
    for i, op in enumerate(ops):
        kind = op[0]
        if kind == OP_FILTER:
            if np.asarray(op[1]).shape[0] > CHAIN_MAX_KSIZE:
                raise ValueError(f"a chain's filter is at most {CHAIN_MAX_KSIZE} x {CHAIN_MAX_KSIZE}")
            x = blur(x, op[1])
        elif kind == OP_RESIZE:
            x = resize(x, op[1], op[2], op[3], op[4])
        elif kind == OP_GAUSS:
            x = gauss_noise(x, op[1], op[2], bool(op[3]))
        elif kind == OP_POISSON:
            x = poisson_noise(x, op[1], op[2], bool(op[3]), table)
        elif kind == OP_DIFFJPEG:
            x = diffjpeg(x, op[1], basis)
        else:
            raise ValueError(f"unknown op {kind}")
        assert x.dtype == np.float32
        if tap == i:
            kept = x
    return finish(x) if tap is None else (finish(x), kept)


# ---------------------------------------------------------------- the folder tool


def degrade_folder(src, dst, recipe="lq", seed=231, backend="host", log=print):
    from PIL import Image
    from instarevive_amd import degrade as D
    rec = D.load_recipe(recipe)
    names = sorted(p for p in os.listdir(src) if p.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    os.makedirs(dst, exist_ok=True)
    ctx = None
    if backend == "gpu":
        import torch
        from instarevive_amd.models import get_context
        ctx = get_context(torch.device("cuda", 0))
    for name in names:
        img = np.asarray(Image.open(os.path.join(src, name)).convert("RGB"))
        p = D.draw(rec, name, img.shape[0], img.shape[1], seed)
        if isinstance(p, D.ChainParams):
            lq = degrade_chain_model(img, p.ops) if ctx is None else D.degrade_chain(ctx, [img], [p])[0]
            Image.fromarray(lq).save(os.path.join(dst, os.path.splitext(name)[0] + ".png"))
            log(f"{name}: {img.shape[1]} x {img.shape[0]}, {p.describe()}")
            continue
        if ctx is None:
            lq = degrade_model(img, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)
        else:
            lq = D.degrade(ctx, [img], [p])[0]
        Image.fromarray(lq).save(os.path.join(dst, os.path.splitext(name)[0] + ".png"))
        log(f"{name}: {img.shape[1]} x {img.shape[0]} -> {p.lw} x {p.lh}, sigma {p.sigma:.2f}, q {p.q}")
    return len(names)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", required=True, help="folder of ground-truth images")
    ap.add_argument("-o", "--output", required=True, help="folder the LQ images are written to as PNG")
    ap.add_argument("--degrade", default="lq", help="`lq` (the constants of the reference's tools/lq.py), `realesrgan` (its second-order validation recipe) or a JSON recipe")
    ap.add_argument("--degrade_seed", type=int, default=231)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    n = degrade_folder(a.input, a.output, a.degrade, a.degrade_seed, a.backend)
    print(f"{n} files -> {a.output}")


if __name__ == "__main__":
    main()
