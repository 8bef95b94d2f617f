"""Inputs and model results shared by tests/test_degrade_cpu.py and tests/test_degrade_gpu.py. The model is tools/degrade_folder.py; the blur
(the expensive step on the host) is computed once per case and the variants (quality x noise x norm) branch off behind the downsample, with
the same step functions degrade_model() chains."""
import functools
import io
import itertools

import numpy as np

from instarevive_amd import degrade as D
from tools import degrade_folder as M

# (name, h, w, scale, kernel arguments (K, sig_x, sig_y, theta, isotropic)). The issue's sizes in both orientations where they are not
# square: 64 x 41 at scale 4 has an even low-resolution height that is no multiple of 16 one way round (10 x 16: the chroma rows replicate
# AFTER the downsample) and a low-resolution width of 10 the other; 37 x 53 at 2.3 gives odd low-resolution sizes (16 x 23, 23 x 16).
CASES = [
    ("48x40_s2.0", 48, 40, 2.0, (41, 3.7, 0.6, 0.9, False)),
    ("37x53_s2.3", 37, 53, 2.3, (41, 1.4, 1.4, 0.0, True)),
    ("53x37_s2.3", 53, 37, 2.3, (41, 1.4, 1.4, 0.0, True)),
    ("64x41_s4.0", 64, 41, 4.0, (41, 2.2, 4.0, -2.0, False)),
    ("41x64_s4.0", 41, 64, 4.0, (41, 2.2, 4.0, -2.0, False)),
    ("96x96_k41_sigma10", 96, 96, 2.0, (41, 10.0, 10.0, 0.0, True)),   # the reflection reaches 20 pixels with weight
    ("256x192_s3.1", 256, 192, 3.1, (41, 0.9, 6.5, 0.4, False)),
]
QUALITIES = (10, 60, 100)
NOISE_SIGMA = 12.5
VARIANTS = list(itertools.product(QUALITIES, (False, True), (M.NORM_NONE, M.NORM_MAX)))   # (q, with noise, norm)


def case(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """Smooth structure plus texture, with the values kept off white so that norm = max changes the bytes."""
    rng = np.random.default_rng([seed, h, w])
    yy, xx = np.mgrid[0:h, 0:w]
    base = 110 + 70 * np.sin(yy / 7.0)[..., None] * np.cos(xx / 5.0)[..., None] * np.array([1.0, 0.8, -0.6])
    img = base + rng.normal(0, 25, (h, w, 3))
    img[h // 3:h // 3 + 4, w // 4:w // 4 + 6] = (235, 20, 20)
    return np.clip(img, 0, 240).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def kernel(args) -> np.ndarray:
    K, sx, sy, th, iso = args
    return D.bivariate_gaussian(K, sx, sy, th, iso)


@functools.lru_cache(maxsize=None)
def noise(lh: int, lw: int) -> np.ndarray:
    return np.random.default_rng([5, lh, lw]).standard_normal((lh, lw, 3), dtype=np.float32)


def low_size(h, w, scale):
    return int(h // scale), int(w // scale)


def params(name):
    """The D.Params of every variant of a case, in VARIANTS' order."""
    _, h, w, scale, kargs = case(name)
    lh, lw = low_size(h, w, scale)
    return [D.Params(kernel(kargs), lh, lw, NOISE_SIGMA if nz else 0.0, q, noise(lh, lw) if nz else None, norm, scale, "") for q, nz, norm in VARIANTS]


@functools.lru_cache(maxsize=None)
def model(name):
    """[(LQ bytes, bytes behind the JPEG step, bytes ahead of it)] of every variant of a case."""
    _, h, w, scale, kargs = case(name)
    lh, lw = low_size(h, w, scale)
    down = M.bilinear(M.blur(M.to_float(image(h, w)), kernel(kargs)), lh, lw)
    out = []
    for q, nz, norm in VARIANTS:
        x = M.add_noise(down, noise(lh, lw), NOISE_SIGMA) if nz else down
        ahead = np.clip(np.rint(x * np.float32(255.0)), 0, 255).astype(np.uint8)
        x, mid = M.jpeg_step(x, q)
        out.append((M.to_bytes(M.bilinear(x, h, w), norm), mid, ahead))
    return out


def pillow_roundtrip(img8: np.ndarray, q: int) -> np.ndarray:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img8).save(buf, format="JPEG", quality=q)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
