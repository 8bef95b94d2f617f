"""The inputs of tests/test_png_runs_cpu.py and tests/test_png_runs_gpu.py, generated: each case is (buffer [n][h][w][3] uint8, vh, vw)."""
import numpy as np

from tests.support import png_model as M

RUN_RESTS = (2, 3, 4, 5, 6, 7, 257, 258, 259, 260, 261, 516, 519)   # R - 1 of the zero runs: around MIN and around the split into 258-pieces


def photo_like(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0 + seed) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8)


def one_row(rests):
    """A one-row image (Paeth is Sub there) whose filtered bytes are, per entry of `rests`, a nonzero byte and then rest + 1 zeros: the channels
    are piecewise constant. The tail is filled up to whole pixels with bytes that form no run."""
    f = [9]
    for i, rest in enumerate(rests):
        f += [1 + i % 7] + [0] * (rest + 1) + [8 + i % 5, 20 + i % 3]
    while len(f) % 3:
        f.append(30 + len(f) % 3)
    f = np.array(f, np.int64).reshape(-1, 3)
    img = (np.cumsum(f, axis=0) % 256).astype(np.uint8)[None]
    filt = M.paeth_filter(img)[0, 1:]
    assert np.array_equal(filt, f.reshape(-1).astype(np.uint8))
    return img


def _padded():
    buf = photo_like(576, 832, 5)[None].copy()
    buf[:, 520:] = 255
    buf[:, :, 776:] = 0
    return buf


def _batch():
    top_flat = photo_like(200, 333, 2)
    top_flat[:100] = (30, 60, 90)
    return np.stack([np.full((200, 333, 3), 200, np.uint8), photo_like(200, 333, 1), top_flat])


def _diagonal():
    yy, xx = np.mgrid[0:20, 0:40]
    return np.repeat((4 * (xx + yy + 1)).astype(np.uint8)[..., None], 3, -1)


def correctness_cases():
    """name -> (buffer, vh, vw). `noise` must fall back in every chunk; `diagonal`'s filtered bytes are all 4, one run per chunk."""
    cases = {
        "one_pixel": (photo_like(1, 1, 3)[None], 1, 1),
        "3x7": (photo_like(3, 7, 3)[None], 3, 7),
        "zeros_17x5": (np.zeros((1, 17, 5, 3), np.uint8), 17, 5),
        "constant_100x120": (np.full((1, 100, 120, 3), 77, np.uint8), 100, 120),
        "photo_64": (photo_like(64, 64, 3)[None], 64, 64),
        "noise": (np.random.default_rng(9).integers(0, 256, (1, 300, 500, 3), dtype=np.uint8), 300, 500),
        "padded": (_padded(), 520, 776),
        "batch_of_three": (_batch(), 200, 333),
        "constant_8x1400": (np.full((1, 8, 1400, 3), 77, np.uint8), 8, 1400),
        "diagonal": (_diagonal()[None], 20, 40),
        "one_row_all": (one_row(RUN_RESTS)[None], 1, None),
    }
    for rest in RUN_RESTS:
        cases[f"one_row_{rest}"] = (one_row([rest, rest])[None], 1, None)
    return {k: (b, vh, vw if vw else b.shape[2]) for k, (b, vh, vw) in cases.items()}


def size_cases():
    """The 512 x 512 images of the size conditions."""
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
    sky = np.rint(np.stack([90 + .25 * yy, 140 + .2 * yy, 220 - .05 * yy + .02 * xx], -1)).astype(np.uint8)
    rng = np.random.default_rng(0)
    pts = rng.integers(0, [512, 512], (12, 2))
    cols = rng.integers(0, 256, (12, 3))
    near = np.argmin((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2, -1)
    photo = M.synthetic(11, 16, 32)
    return {
        "constant": np.full((512, 512, 3), 77, np.uint8),
        "sky": sky,
        "flat_regions": cols[near].astype(np.uint8),
        "photo": photo,
        "sky_over_photo": np.concatenate((sky[:256], photo[:256])),
    }
