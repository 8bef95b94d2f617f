"""The numpy statement of Pillow's 8-bit resampling passes (Resample.c: ImagingResampleHorizontal_8bpc / Vertical_8bpc), given the bounds and
coefficient tables of an ir_resample_plan: ss = 2^21 + sum(pixel * k) in integers, out = clamp(ss >> 22, 0, 255), horizontal pass first,
the image between the passes uint8, a pass whose lengths are equal skipped. What csrc/resample.hip has to reproduce byte for byte."""
import ctypes as C

import numpy as np

PRECISION_BITS = 22
HEADER = 16
MAGIC = 0x52535038
BICUBIC, LANCZOS = 0, 1


def plan(lib, in_h, in_w, out_h, out_w, flt) -> np.ndarray:
    """ir_resample_plan's int32 array."""
    nbytes = int(lib.ir_resample_plan_bytes(in_h, in_w, out_h, out_w, flt))
    assert nbytes >= 4 * HEADER and nbytes % 4 == 0, nbytes
    buf = np.zeros(nbytes // 4, np.int32)
    assert lib.ir_resample_plan(in_h, in_w, out_h, out_w, flt, C.c_void_p(buf.ctypes.data), nbytes) == 0
    return buf


def tables(p: np.ndarray):
    """-> ((bounds_h [out_w][2], coeffs_h [out_w][ksize_h]) or None, the same of the vertical pass or None)."""
    assert p[0] == MAGIC and p[12] == p.size
    _, in_h, in_w, out_h, out_w = (int(v) for v in p[:5])
    ks_h, ks_v = int(p[6]), int(p[7])
    hor = ver = None
    if in_w != out_w:
        hor = (p[p[8]:p[8] + 2 * out_w].reshape(out_w, 2), p[p[9]:p[9] + out_w * ks_h].reshape(out_w, ks_h))
    if in_h != out_h:
        ver = (p[p[10]:p[10] + 2 * out_h].reshape(out_h, 2), p[p[11]:p[11] + out_h * ks_v].reshape(out_h, ks_v))
    return hor, ver


def one_pass(img: np.ndarray, bounds: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
    """Resample axis 0 of img [len][...] uint8."""
    src = img.astype(np.int64)
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    for i, (lo, cnt) in enumerate(bounds):
        k = coeffs[i, :cnt].astype(np.int64)
        ss = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[lo:lo + cnt], axes=(0, 0))
        assert np.abs(ss).max() < 2 ** 31   # the device sums in int32
        out[i] = np.clip(ss >> PRECISION_BITS, 0, 255)
    return out


def resample(img: np.ndarray, p: np.ndarray) -> np.ndarray:
    """img [in_h][in_w][3] uint8 -> [out_h][out_w][3] by the plan p."""
    assert img.dtype == np.uint8 and img.shape[:2] == (p[1], p[2])
    hor, ver = tables(p)
    if hor is not None:
        img = one_pass(img.transpose(1, 0, 2), *hor).transpose(1, 0, 2)
    if ver is not None:
        img = one_pass(img, *ver)
    return np.ascontiguousarray(img)
