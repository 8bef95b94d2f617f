"""IL-NIQE of results on the device (ir_ilniqe_stats, csrc/ilniqe.hip): the no-reference metric that the reference's evaluate_img.py keeps commented
out next to `niqe` (pyiqa's `ilniqe`; tools/evaluate_ilniqe.py restates it in numpy fp64 and is the model). The pixel work - the resize to
524 x 524, the 109 planes of both scales (twelve log-Gabor responses through a dense fp64 DFT on the MFMA, 54 derivative convolutions) and the
558 statistics of every block, Weibull fits included - runs behind the network on the uint8 result that is in device memory anyway; the
asymmetric generalised Gaussian fits (features_from_stats), the projection on the principal vectors and the score against the user's template
(score) are host work on a few hundred KB, done where the scores are read and not between launches.

tables() makes the fixed tables in fp64 (the windows, the derivative taps, the filter banks), configure() uploads and binds them, plan() caches
the resize tables of an input size, queue_stats() puts the call on the current stream, IlniqeSlot holds the statistics of one staging slot
(device side and page-locked, like niqe.NiqeSlot), load_params() reads ILNIQE_templateModel.mat or an .npz. queue_dft2() / queue_weibull() and
dft2() / weibull_fit() reach the two building blocks on their own (ir_op_dft2_f64, ir_op_weibull_fit).
"""
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .niqe import _alpha_of, _lg
from .slots import Pooled, spans

SIZE, USED, BLOCK = 524, 504, 84
BLOCKS = 36
STATS = 558          # doubles per scale and block: 30 + 78 * 6 + 6 + 54
ROW = 2 * BLOCKS * STATS
FEATURES = 468
INF_CONST = 10000.0
SIZES = (252, 504)
WEIBULL_MAX = 7056   # one 84 x 84 block
NAMES = ("mu_prisparam", "cov_prisparam", "meanOfSampleData", "principleVectors")


class IlniqeError(ValueError):
    pass


def load_params(path: str):
    """(mu_prisparam [d], cov_prisparam [d][d], meanOfSampleData [468], principleVectors [468][d]) as float64 from the user's
    ILNIQE_templateModel.mat (key templateModel, a 1 x 4 cell) or an .npz with those four names; d comes from the file. Anything else raises
    IlniqeError naming the file."""
    try:
        if str(path).lower().endswith(".npz"):
            with np.load(path) as z:
                missing = [k for k in NAMES if k not in z.files]
                if missing:
                    raise IlniqeError(f"--ilniqe_params {path}: {' and '.join(missing)} missing (IL-NIQE's template: mu_prisparam [d], cov_prisparam [d][d], "
                                      f"meanOfSampleData [468], principleVectors [468][d])")
                got = [np.asarray(z[k], np.float64) for k in NAMES]
        else:
            from scipy.io import loadmat
            m = loadmat(str(path))
            if "templateModel" not in m or np.asarray(m["templateModel"]).size != 4 or np.asarray(m["templateModel"]).dtype != object:
                raise IlniqeError(f"--ilniqe_params {path}: no 1 x 4 cell templateModel (mu_prisparam, cov_prisparam, meanOfSampleData, principleVectors)")
            got = [np.asarray(v, np.float64) for v in np.asarray(m["templateModel"]).reshape(-1)]
    except IlniqeError:
        raise
    except Exception as e:   # scipy raises its own MatReadError for a file that is no .mat
        raise IlniqeError(f"--ilniqe_params {path}: cannot be read ({e})") from None
    mu, cov, mean_s, pv = got
    d = mu.size
    if d < 1 or mu.ndim > 2 or max(mu.shape, default=0) != d or cov.shape != (d, d) or mean_s.size != FEATURES or mean_s.ndim > 2 or pv.shape != (FEATURES, d):
        raise IlniqeError(f"--ilniqe_params {path}: mu_prisparam is {mu.shape}, cov_prisparam {cov.shape}, meanOfSampleData {mean_s.shape} and principleVectors "
                          f"{pv.shape}; d values, d x d, 468 values and 468 x d are needed")
    if not all(np.isfinite(v).all() for v in got):
        raise IlniqeError(f"--ilniqe_params {path}: the template holds NaN or infinity")
    return mu.reshape(d).copy(), cov.copy(), mean_s.reshape(FEATURES).copy(), pv.copy()


# ---------------------------------------------------------------------------------------------------------------- the fixed tables
def gaussian_window(size: int, sigma: float) -> np.ndarray:
    """MATLAB's fspecial('gaussian', size, sigma): entries below eps * max zeroed, divided by the sum taken in row-major order."""
    c = (size - 1) / 2.0
    g = np.array([[math.exp(-((i - c) ** 2 + (j - c) ** 2) / (2.0 * sigma * sigma)) for j in range(size)] for i in range(size)])
    g[g < np.finfo(np.float64).eps * g.max()] = 0.0
    total = 0.0
    for v in g.reshape(-1):
        total += float(v)
    return g / total


def derivative_taps(scale: int) -> np.ndarray:
    """[2][11]: x g(x) and g(x) on -5 .. 5 for sigma = 1.66 / scale^0.28."""
    sg = 1.66 / scale ** 0.28
    half = int(math.ceil(3.0 * sg))
    g = np.array([math.exp(-(t * t) / (2.0 * sg * sg)) for t in range(-half, half + 1)])
    return np.stack([np.arange(-half, half + 1) * g, g])


def log_gabor_bank(n: int, scale: int) -> np.ndarray:
    """[12][n][n]: Kovesi's log-Gabor times angular spread in (scale, orientation) order on the ifftshifted frequency grid, times the low-pass
    1 / (1 + (r / 0.45)^30), DC zeroed (the definition's step 3)."""
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
            bank[4 * k + o] = radial * np.exp(-np.abs(np.arctan2(ds, dc)) ** 2 / (2.0 * theta_sigma ** 2))
    return bank


_tables = None


def tables() -> Dict[str, np.ndarray]:
    """The float64 tables ir_ilniqe_configure binds, by tensor name."""
    global _tables
    if _tables is None:
        _tables = {"ilniqe.win5": gaussian_window(5, 5.0 / 6.0), "ilniqe.win6": gaussian_window(6, 0.9),
                   "ilniqe.taps": np.stack([derivative_taps(1), derivative_taps(2)]),
                   "ilniqe.bank504": log_gabor_bank(504, 1), "ilniqe.bank252": log_gabor_bank(252, 2)}
    return _tables


def configure(ctx) -> None:
    """Upload tables() and bind them (ir_ilniqe_configure, which adds the twiddle matrices): 42 MB of device memory. The calls of this module
    refuse a context without them."""
    for name, t in tables().items():
        ctx.upload(name, torch.from_numpy(np.ascontiguousarray(t, np.float64)))
    ctx.check(ctx.lib.ir_ilniqe_configure(ctx.h), "ir_ilniqe_configure")
    ctx.__dict__["_ilniqe_plans"] = {}


def configured(ctx) -> bool:
    return "_ilniqe_plans" in ctx.__dict__


def taps_of(n_in: int) -> int:
    """The taps per output of the resize along an axis of n_in pixels: ceil(width) + 2, width = 4 / scale when scale = 524 / n_in < 1, else 4."""
    scale = SIZE / n_in
    return int(math.ceil(4.0 / scale if scale < 1.0 else 4.0)) + 2


def plan_host(h: int, w: int) -> np.ndarray:
    """ir_ilniqe_plan's bytes for an h x w input as a uint8 array."""
    lib = L.load_library()
    n = int(lib.ir_ilniqe_plan_bytes(h, w))
    if n < 0:
        raise IlniqeError(f"IL-NIQE needs an image of at least 2 x 2; this one is {h} x {w}")
    buf = np.zeros((n + 7) // 8, np.float64)   # 8-byte aligned
    if lib.ir_ilniqe_plan(h, w, C.c_void_p(buf.ctypes.data), n) != 0:
        raise RuntimeError("ir_ilniqe_plan failed")
    return buf.view(np.uint8)[:n]


def plan_arrays(h: int, w: int):
    """((idx0 [524][P0], w0 [524][P0]), (idx1 [524][P1], w1 [524][P1])) of plan_host(h, w): what a host model reads."""
    raw = plan_host(h, w)
    p0, p1 = taps_of(h), taps_of(w)
    i1 = SIZE * p0 * 4
    o0 = (i1 + SIZE * p1 * 4 + 7) & ~7
    o1 = o0 + SIZE * p0 * 8
    idx0, idx1 = raw[:i1].view(np.int32).reshape(SIZE, p0), raw[i1:i1 + SIZE * p1 * 4].view(np.int32).reshape(SIZE, p1)
    w0, w1 = raw[o0:o1].view(np.float64).reshape(SIZE, p0), raw[o1:o1 + SIZE * p1 * 8].view(np.float64).reshape(SIZE, p1)
    return (idx0.astype(np.int64), w0.copy()), (idx1.astype(np.int64), w1.copy())


def plan(ctx, h: int, w: int) -> torch.Tensor:
    """The device copy of the resize tables of an h x w input, cached per context and size (as resample.Plans caches its plans)."""
    cache = ctx.__dict__.setdefault("_ilniqe_plans", {})
    if (h, w) not in cache:
        cache[(h, w)] = torch.from_numpy(plan_host(h, w).copy()).to(ctx.device)
    return cache[(h, w)]


def ws_bytes(n: int, h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_ILNIQE, n, h, w, 0, 0, 0))


def queue_stats(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_ilniqe_stats on the current stream: the n images of h x w at device address img ([n][rows][pitch] bytes, RGB8). out: a contiguous
    float64 device tensor of n x 2 x 36 x 558 values - by default the context's own buffer, whose page-locked twin fetch_stats() fills. The
    scratch is the context's workspace. The plan of a new size is uploaded here, before the call is queued."""
    count = n * ROW
    if out is None:
        buf = ctx.__dict__.get("_ilniqe_stats")
        if buf is None or buf[0].numel() < count:
            buf = ctx.__dict__["_ilniqe_stats"] = (torch.zeros((count,), dtype=torch.float64, device=ctx.device), torch.zeros((count,), dtype=torch.float64).pin_memory())
        out = buf[0][:count]
    if out.dtype != torch.float64 or out.numel() < count or not out.is_contiguous():
        raise ValueError("queue_stats: out must be a contiguous float64 tensor of n x 2 x 36 x 558 values")
    pl = plan(ctx, h, w)
    ws = ctx.workspace(max(ws_bytes(n, h, w), 256))
    ctx.check(ctx.lib.ir_ilniqe_stats(ctx.h, ctx.stream(), C.c_void_p(img), rows, pitch, n, h, w, L.ptr(pl), C.c_void_p(out.data_ptr()), L.ptr(ws), ws.numel()),
              "ir_ilniqe_stats")
    return out


def fetch_stats(ctx, n: int) -> np.ndarray:
    """[n][2][36][558] of the last queue_stats(out=None): downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_ilniqe_stats"]
    host[:n * ROW].copy_(dev[:n * ROW], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return host[:n * ROW].numpy().reshape(n, 2, BLOCKS, STATS).copy()


# ---------------------------------------------------------------------------------------------------------------- the host part
def _aggd(six: np.ndarray, count: float):
    """[..., 6] -> (alpha, beta_l, beta_r, mean): NIQE's fit from the six numbers."""
    cl, cr, sl, sr, sa, ss = (six[..., k] for k in range(6))
    ls, rs = np.sqrt(sl / cl), np.sqrt(sr / cr)
    g = ls / rs
    rhat = (sa / count) ** 2 / (ss / count)
    rn = rhat * (g ** 3 + 1.0) * (g + 1.0) / (g ** 2 + 1.0) ** 2
    alpha = _alpha_of(rn)
    sc = np.sqrt(np.exp(_lg(1.0 / alpha) - _lg(3.0 / alpha)))
    bl, br = ls * sc, rs * sc
    return alpha, bl, br, (br - bl) * np.exp(_lg(2.0 / alpha) - _lg(1.0 / alpha))


def features_from_stats(stats: np.ndarray) -> np.ndarray:
    """[2][36][558] (one image of ir_ilniqe_stats) -> [36][468]: per scale and block 18 features of plane 0, (lambda, k) of planes 1-3, mean and
    variance of planes 4-6, alpha and (beta_l + beta_r) / 2 of planes 7-84, (lambda, k) of planes 85-108. A field without negative or without
    positive values gives NaN, which score() handles."""
    stats = np.asarray(stats, np.float64)
    if stats.shape != (2, BLOCKS, STATS):
        raise IlniqeError(f"features_from_stats: [2][36][558] is needed, got {stats.shape}")
    feat = np.empty((BLOCKS, FEATURES))
    with np.errstate(all="ignore"):
        for s in range(2):
            count = float((BLOCK // (s + 1)) ** 2)
            st = stats[s]
            a, bl, br, mean = _aggd(st[:, :30].reshape(BLOCKS, 5, 6), count)
            cols = [a[:, 0], (bl[:, 0] + br[:, 0]) / 2.0]
            for f in range(1, 5):
                cols += [a[:, f], mean[:, f], bl[:, f], br[:, f]]
            wb = st[:, 504:558].reshape(BLOCKS, 27, 2)
            for p in range(3):
                cols += [wb[:, p, 1], wb[:, p, 0]]
            cols += [st[:, 498 + i] for i in range(6)]
            a, bl, br, _ = _aggd(st[:, 30:498].reshape(BLOCKS, 78, 6), count)
            for p in range(78):
                cols += [a[:, p], (bl[:, p] + br[:, p]) / 2.0]
            for p in range(3, 27):
                cols += [wb[:, p, 1], wb[:, p, 0]]
            feat[:, 234 * s:234 * s + 234] = np.stack(cols, 1)
    return feat


def score(feat: np.ndarray, params) -> float:
    """The IL-NIQE score of a feature matrix [36][468] against the template (load_params): values above 10000 set to 10000, c = P^T (f - mean) per
    block, NaN entries replaced by the column's nan-mean, the unbiased covariance of the blocks without NaN, the mean over the blocks of
    sqrt(d pinv((cov_pris + cov_d) / 2) d^T) with d = c - mu_pris. IlniqeError with fewer than two complete blocks."""
    mu_p, cov_p, mean_s, pv = params
    feat = np.asarray(feat, np.float64)
    with np.errstate(all="ignore"):
        feat = np.where(feat > INF_CONST, INF_CONST, feat)
        c = (feat - mean_s.reshape(1, -1)) @ pv
        nan = np.isnan(c)
        ok = ~nan.any(axis=1)
        if int(ok.sum()) < 2:
            raise IlniqeError(f"IL-NIQE needs two complete feature rows; {int(ok.sum())} of {feat.shape[0]} blocks gave one")
        mu_d = np.where(nan, 0.0, c).sum(axis=0) / (~nan).sum(axis=0)
    c = np.where(nan, mu_d[None, :], c)
    rows = c[ok]
    cen = rows - rows.mean(axis=0)
    cov_d = cen.T @ cen / (rows.shape[0] - 1)
    inv = np.linalg.pinv((np.asarray(cov_p, np.float64) + cov_d) / 2.0)
    d = c - np.asarray(mu_p, np.float64).reshape(1, -1)
    return float(np.mean(np.sqrt(np.einsum("bi,ij,bj->b", d, inv, d))))


def score_or_nan(stats: np.ndarray, params) -> float:
    """score(features_from_stats(stats)), NaN where the image has no score (what the pipeline returns for such an image)."""
    try:
        return score(features_from_stats(stats), params)
    except IlniqeError:
        return float("nan")


def stats_arrays(ctx, img: np.ndarray) -> np.ndarray:
    """[2][36][558] of an HWC uint8 RGB array: upload, one call, wait."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise IlniqeError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if min(h, w) < 2:
        raise IlniqeError(f"IL-NIQE needs an image of at least 2 x 2; this one is {h} x {w}")
    dev = torch.from_numpy(img).to(ctx.device)
    queue_stats(ctx, dev.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_stats(ctx, 1)[0]


def score_arrays(ctx, img: np.ndarray, params) -> float:
    """IL-NIQE of an HWC uint8 RGB array. For tools and tests; the pipeline scores in place."""
    return score(features_from_stats(stats_arrays(ctx, img)), params)


class IlniqeSlot(Pooled):
    """The block statistics of one staging slot's batch: a float64 device buffer [row][2][36][558] and its page-locked twin; both grow on demand
    and are reused by the next batch of the slot. A row is an image of the batch: the predictions first, then - when asked for - the stage-1
    images. Every image is resized to 524 x 524 first, so every row has the same length; an image below 2 pixels on an edge has no score (NaN)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d_stats = self.h_stats = None
        self.params = None
        self.shapes: List[Tuple[int, int]] = []
        self.used = 0

    def plan(self, finals: Sequence[Tuple[int, int]], params, copies: int = 1) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        self.params = params
        self.shapes = [tuple(int(v) for v in f) for f in finals] * copies
        self.used = len(self.shapes) * ROW
        if self.d_stats is None or self.d_stats.numel() < self.used:
            self.d_stats = torch.zeros((self.used,), dtype=torch.float64, device=self.ctx.device)
            self.h_stats = torch.zeros((self.used,), dtype=torch.float64).pin_memory()

    def reserve(self) -> None:
        """Grow the context's workspace to what the largest call of this batch may need and upload the plans of its sizes, before anything of the
        batch is queued."""
        sizes = [s for s in self.shapes if min(s) >= 2]
        for h, w in set(sizes):
            plan(self.ctx, h, w)
        self.ctx.workspace(max([ws_bytes(1, h, w) for h, w in sizes] + [256]))

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """ir_ilniqe_stats of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current
        stream. results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            if min(gh, gw) < 2:
                continue
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            at = (first + i) * ROW
            queue_stats(self.ctx, img, rows, pitch, k - i, gh, gw, self.d_stats[at:at + (k - i) * ROW])

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's statistics on the current stream."""
        if self.used:
            self.h_stats[:self.used].copy_(self.d_stats[:self.used], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(ilniqe,) of rows first .. first + count - 1 after the download has completed: the host part (the fits and the score) runs here. NaN
        for an image without a score."""
        host = self.h_stats.numpy()
        out = []
        for i, (h, w) in enumerate(self.shapes[first:first + count]):
            at = (first + i) * ROW
            out.append((score_or_nan(host[at:at + ROW].reshape(2, BLOCKS, STATS), self.params) if min(h, w) >= 2 else float("nan"),))
        return out


# ---------------------------------------------------------------------------------------------------------------- the two building blocks
def dft_ws_bytes(size: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_ILNIQE_DFT, 1, size, size, 0, 0, 0))


def queue_dft2(ctx, re: torch.Tensor, im: Optional[torch.Tensor], inverse: bool, out_re: torch.Tensor, out_im: torch.Tensor) -> None:
    """ir_op_dft2_f64 on the current stream: contiguous float64 device tensors [size][size]; im may be None (a real input). The outputs must
    not overlap the inputs. The scratch is the context's workspace."""
    size = re.shape[-1]
    for t in (re, im, out_re, out_im):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (size, size) or not t.is_contiguous()):
            raise IlniqeError(f"queue_dft2: contiguous float64 tensors of {size} x {size} are needed")
    ws = ctx.workspace(max(dft_ws_bytes(size), 256))
    ctx.check(ctx.lib.ir_op_dft2_f64(ctx.h, ctx.stream(), L.ptr(re), L.ptr(im), size, int(bool(inverse)), L.ptr(out_re), L.ptr(out_im), L.ptr(ws), ws.numel()),
              "ir_op_dft2_f64")


def queue_weibull(ctx, x: torch.Tensor, out: torch.Tensor) -> None:
    """ir_op_weibull_fit on the current stream: x [rows][count] and out [rows][2] (k, lambda), contiguous float64 device tensors."""
    if x.dtype != torch.float64 or x.ndim != 2 or not x.is_contiguous() or out.dtype != torch.float64 or tuple(out.shape) != (x.shape[0], 2) or not out.is_contiguous():
        raise IlniqeError("queue_weibull: x [rows][count] and out [rows][2] as contiguous float64 tensors are needed")
    ctx.check(ctx.lib.ir_op_weibull_fit(ctx.h, ctx.stream(), L.ptr(x), x.shape[0], x.shape[1], L.ptr(out)), "ir_op_weibull_fit")


def dft2(ctx, re: np.ndarray, im: Optional[np.ndarray] = None, inverse: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(re, im) of the 2-D DFT of a 252 x 252 or 504 x 504 float64 array."""
    re = np.ascontiguousarray(re, np.float64)
    if re.ndim != 2 or re.shape[0] != re.shape[1] or re.shape[0] not in SIZES:
        raise IlniqeError(f"dft2: 252 x 252 or 504 x 504 is needed, got {re.shape}")
    d_re = torch.from_numpy(re).to(ctx.device)
    d_im = None if im is None else torch.from_numpy(np.ascontiguousarray(im, np.float64)).to(ctx.device)
    o_re, o_im = torch.empty_like(d_re), torch.empty_like(d_re)
    queue_dft2(ctx, d_re, d_im, inverse, o_re, o_im)
    return o_re.cpu().numpy(), o_im.cpu().numpy()


def weibull_fit(ctx, x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(k [rows], lambda [rows]) of rows of positive float64 values [rows][count], count 2 .. 7056."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2 or not 2 <= x.shape[1] <= WEIBULL_MAX or x.shape[0] < 1:
        raise IlniqeError(f"weibull_fit: [rows][2 .. {WEIBULL_MAX}] is needed, got {x.shape}")
    d_x = torch.from_numpy(x).to(ctx.device)
    out = torch.empty((x.shape[0], 2), dtype=torch.float64, device=ctx.device)
    queue_weibull(ctx, d_x, out)
    o = out.cpu().numpy()
    return o[:, 0].copy(), o[:, 1].copy()
