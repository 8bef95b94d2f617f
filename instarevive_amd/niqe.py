"""NIQE of results on the device (ir_niqe_stats, csrc/niqe.hip): the no-reference metric of the reference's evaluate_img.py that is classical image
statistics and no pretrained network (pyiqa's `niqe`; tools/evaluate_niqe.py restates it in numpy fp64 and is the model). The pixel work - luma,
the half-size plane, the MSCN values of both scales and the thirty sums of every block - runs behind the network on the uint8 result that is in
device memory anyway; the asymmetric generalised Gaussian fit of every block (features_from_stats) and the score against the user's pristine
parameters (score) are host work on a few KB, done where the scores are read and not between launches.

queue_stats() puts the call on the current stream, NiqeSlot holds the statistics of one staging slot (device side and page-locked, grown on demand,
like metrics.ScoreSlot), load_params() reads niqe_modelparameters.mat or an .npz.
"""
import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

BLOCK = 96        # a block at scale 1; images below 96 x 96 have no NIQE
FEATURES = 36
STATS = 2 * 5 * 6   # doubles per block: [scale][field][six numbers]


class NiqeError(ValueError):
    pass


def load_params(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(mu_prisparam [36], cov_prisparam [36][36]) as float64 from the user's niqe_modelparameters.mat (scipy.io.loadmat) or an .npz with those
    two keys. A missing key or another shape raises NiqeError naming the file."""
    try:
        if str(path).lower().endswith(".npz"):
            with np.load(path) as z:
                d = {k: z[k] for k in z.files}
        else:
            from scipy.io import loadmat
            d = loadmat(str(path))
    except Exception as e:   # scipy raises its own MatReadError for a file that is no .mat
        raise NiqeError(f"--niqe_params {path}: cannot be read ({e})") from None
    missing = [k for k in ("mu_prisparam", "cov_prisparam") if k not in d]
    if missing:
        raise NiqeError(f"--niqe_params {path}: {' and '.join(missing)} missing (NIQE's pristine parameters: mu_prisparam [36], cov_prisparam [36][36])")
    mu, cov = np.asarray(d["mu_prisparam"], np.float64), np.asarray(d["cov_prisparam"], np.float64)
    if mu.size != FEATURES or mu.ndim > 2 or cov.shape != (FEATURES, FEATURES):
        raise NiqeError(f"--niqe_params {path}: mu_prisparam is {mu.shape} and cov_prisparam {cov.shape}; 36 values and 36 x 36 are needed")
    if not (np.isfinite(mu).all() and np.isfinite(cov).all()):
        raise NiqeError(f"--niqe_params {path}: the parameters hold NaN or infinity")
    return mu.reshape(FEATURES).copy(), cov.copy()


def window() -> np.ndarray:
    """The 7 x 7 window of the kernels (ir_niqe_window) as a float64 array."""
    buf = (C.c_double * 49)()
    if L.load_library().ir_niqe_window(buf) != 0:
        raise RuntimeError("ir_niqe_window failed")
    return np.array(buf, dtype=np.float64).reshape(7, 7)


def ws_bytes(n: int, h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_NIQE, n, h, w, 0, 0, 0))


def blocks_of(h: int, w: int) -> int:
    return (h // BLOCK) * (w // BLOCK)


def queue_stats(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_niqe_stats on the current stream: the top-left (h // 96 * 96) x (w // 96 * 96) rectangle of the n images at device address img
    ([n][rows][pitch] bytes, RGB8). out: a contiguous float64 device tensor of n x 2 x blocks x 5 x 6 values - by default the context's own buffer,
    whose page-locked twin fetch_stats() fills. The scratch is the context's workspace (see metrics.queue_scores)."""
    count = n * blocks_of(h, w) * STATS
    if out is None:
        buf = ctx.__dict__.get("_niqe_stats")
        if buf is None or buf[0].numel() < count:
            cap = max(count, 64 * STATS)
            buf = ctx.__dict__["_niqe_stats"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:count]
    if out.dtype != torch.float64 or out.numel() < count or not out.is_contiguous():
        raise ValueError("queue_stats: out must be a contiguous float64 tensor of n x 2 x blocks x 5 x 6 values")
    ws = ctx.workspace(max(ws_bytes(n, h, w), 256))
    ctx.check(ctx.lib.ir_niqe_stats(ctx.h, ctx.stream(), C.c_void_p(img), rows, pitch, n, h, w, C.c_void_p(out.data_ptr()), L.ptr(ws), ws.numel()), "ir_niqe_stats")
    return out


def fetch_stats(ctx, n: int, h: int, w: int) -> np.ndarray:
    """[n][2][blocks][5][6] of the last queue_stats(out=None): downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_niqe_stats"]
    count = n * blocks_of(h, w) * STATS
    host[:count].copy_(dev[:count], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return host[:count].numpy().reshape(n, 2, blocks_of(h, w), 5, 6).copy()


# ---------------------------------------------------------------------------------------------------------------- the host part
_lgamma = np.frompyfunc(math.lgamma, 1, 1)
_tables = None


def _lg(x: np.ndarray) -> np.ndarray:
    return _lgamma(x).astype(np.float64)


def gam_tables() -> Tuple[np.ndarray, np.ndarray]:
    """(gam, r_gam): gam = arange(0.2, 10.001, 0.001) and r_gam = exp(2 lgamma(2/gam) - lgamma(1/gam) - lgamma(3/gam)), which is strictly
    increasing (smallest step 1.67e-6), so the nearest entry is found by bisection."""
    global _tables
    if _tables is None:
        gam = np.arange(0.2, 10.001, 0.001)
        _tables = (gam, np.exp(2.0 * _lg(2.0 / gam) - _lg(1.0 / gam) - _lg(3.0 / gam)))
    return _tables


def _alpha_of(rn: np.ndarray) -> np.ndarray:
    """gam[argmin |r_gam - rn|], the first minimum winning; NaN and infinity take entry 0 (what argmin gives when every distance is alike)."""
    gam, r = gam_tables()
    safe = np.where(np.isfinite(rn), rn, -np.inf)
    hi = np.clip(np.searchsorted(r, safe, side="left"), 0, len(r) - 1)
    lo = np.clip(hi - 1, 0, len(r) - 1)
    with np.errstate(invalid="ignore"):
        take_lo = np.abs(r[lo] - safe) <= np.abs(r[hi] - safe)
    return gam[np.where(take_lo, lo, hi)]


def features_from_stats(stats: np.ndarray) -> np.ndarray:
    """[2][blocks][5][6] (one image of ir_niqe_stats) -> [blocks][36]: per scale and block the asymmetric generalised Gaussian fit of the five
    fields. A field without negative or without positive values (an all-zero block) gives NaN, which score() handles."""
    stats = np.asarray(stats, np.float64)
    if stats.ndim != 4 or stats.shape[0] != 2 or stats.shape[2:] != (5, 6):
        raise NiqeError(f"features_from_stats: [2][blocks][5][6] is needed, got {stats.shape}")
    nb = stats.shape[1]
    feat = np.empty((nb, FEATURES))
    with np.errstate(all="ignore"):
        for s in range(2):
            n = float((BLOCK // (s + 1)) ** 2)
            cl, cr, sl, sr, sa, ss = (stats[s, :, :, k] for k in range(6))
            ls, rs = np.sqrt(sl / cl), np.sqrt(sr / cr)
            g = ls / rs
            rhat = (sa / n) ** 2 / (ss / n)
            rn = rhat * (g ** 3 + 1.0) * (g + 1.0) / (g ** 2 + 1.0) ** 2
            alpha = _alpha_of(rn)
            scale = np.sqrt(np.exp(_lg(1.0 / alpha) - _lg(3.0 / alpha)))
            bl, br = ls * scale, rs * scale
            mean = (br - bl) * np.exp(_lg(2.0 / alpha) - _lg(1.0 / alpha))
            cols = [alpha[:, 0], (bl[:, 0] + br[:, 0]) / 2.0]
            for f in range(1, 5):
                cols += [alpha[:, f], mean[:, f], bl[:, f], br[:, f]]
            feat[:, 18 * s:18 * s + 18] = np.stack(cols, 1)
    return feat


def score(feat: np.ndarray, params) -> float:
    """The NIQE score of a feature matrix [blocks][36] against (mu_prisparam, cov_prisparam): column means over the non-NaN entries, the unbiased
    covariance of the rows without NaN, sqrt(d pinv((cov_pris + cov_d) / 2) d^T). NiqeError with fewer than two complete rows."""
    mu_p, cov_p = params
    feat = np.asarray(feat, np.float64)
    nan = np.isnan(feat)
    rows = feat[~nan.any(axis=1)]
    if rows.shape[0] < 2:
        raise NiqeError(f"NIQE needs two complete feature rows; {rows.shape[0]} of {feat.shape[0]} blocks gave one")
    mu_d = np.where(nan, 0.0, feat).sum(axis=0) / (~nan).sum(axis=0)
    cov_d = np.cov(rows, rowvar=False, ddof=1)
    d = (np.asarray(mu_p, np.float64).reshape(FEATURES) - mu_d).reshape(1, FEATURES)
    inv = np.linalg.pinv((np.asarray(cov_p, np.float64) + cov_d) / 2.0)
    return float(np.sqrt((d @ inv @ d.T)[0, 0]))


def score_or_nan(stats: np.ndarray, params) -> float:
    """score(features_from_stats(stats)), NaN where the image has no score (what the pipeline returns for such an image)."""
    try:
        return score(features_from_stats(stats), params)
    except NiqeError:
        return float("nan")


def stats_arrays(ctx, img: np.ndarray) -> np.ndarray:
    """[2][blocks][5][6] of an HWC uint8 RGB array: upload, one call, wait."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise NiqeError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if min(h, w) < BLOCK:
        raise NiqeError(f"NIQE needs at least one 96 x 96 block; the image is {h} x {w}")
    dev = torch.from_numpy(img).to(ctx.device)
    queue_stats(ctx, dev.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_stats(ctx, 1, h, w)[0]


def score_arrays(ctx, img: np.ndarray, params) -> float:
    """NIQE of an HWC uint8 RGB array. For tools and tests; the pipeline scores in place."""
    return score(features_from_stats(stats_arrays(ctx, img)), params)


class NiqeSlot(Pooled):
    """The block statistics of one staging slot's batch: a flat float64 device buffer and its page-locked twin, [row][2][blocks][5][6] packed without
    gaps (images differ in size, so rows differ in length); both grow on demand and are reused by the next batch of the slot. A row is an image of
    the batch: the predictions first, then - when asked for - the stage-1 images. Images below 96 pixels on an edge have no blocks: nothing is
    launched for them and their score is NaN."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d_stats = self.h_stats = None
        self.params = None
        self.shapes: List[Tuple[int, int]] = []
        self.offsets: List[int] = []
        self.used = 0

    def plan(self, finals: Sequence[Tuple[int, int]], params, copies: int = 1) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        self.params = params
        self.shapes = [tuple(int(v) for v in f) for f in finals] * copies
        self.offsets, at = [], 0
        for h, w in self.shapes:
            self.offsets.append(at)
            at += blocks_of(h, w) * STATS
        self.used = at
        if self.d_stats is None or self.d_stats.numel() < at:
            cap = max(at, 64 * STATS)
            self.d_stats = torch.zeros((cap,), dtype=torch.float64, device=self.ctx.device)
            self.h_stats = torch.zeros((cap,), dtype=torch.float64).pin_memory()

    def reserve(self) -> None:
        """Grow the context's workspace to what the largest call of this batch may need (all images of one size in one call), before anything of
        the batch is queued."""
        n = len(self.shapes)
        self.ctx.workspace(max([ws_bytes(n, h, w) for h, w in self.shapes if min(h, w) >= BLOCK] + [256]))

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """ir_niqe_stats of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current stream.
        results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            if min(gh, gw) < BLOCK:
                continue
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            at = self.offsets[first + i]
            queue_stats(self.ctx, img, rows, pitch, k - i, gh, gw, self.d_stats[at:at + (k - i) * blocks_of(gh, gw) * STATS])

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's statistics on the current stream."""
        if self.used:
            self.h_stats[:self.used].copy_(self.d_stats[:self.used], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(niqe,) of rows first .. first + count - 1 after the download has completed: the host part (the fits and the score) runs here. NaN for an
        image without a score (below 96 pixels on an edge, or fewer than two complete feature rows)."""
        host = self.h_stats.numpy()
        out = []
        for (h, w), at in zip(self.shapes[first:first + count], self.offsets[first:first + count]):
            nb = blocks_of(h, w)
            out.append((score_or_nan(host[at:at + nb * STATS].reshape(2, nb, 5, 6), self.params) if nb else float("nan"),))
        return out
