"""Low-quality inputs synthesised from ground truth (ir_degrade, csrc/degrade.hip): the host side. The reference makes its LQ sets with
tools/lq.py, the first-order chain of dataset/codeformer.py:CodeformerDataset.__getitem__ (:140-163) - blur, bilinear downsample, noise, JPEG,
bilinear resize back - with OpenCV and a second folder of files; here the ground truth goes to the device and the LQ image is made there
(tools/degrade_folder.py is the definition, in numpy).

A recipe holds the ranges the parameters are drawn from (LQ_RECIPE: the constants of tools/lq.py; a JSON file with CodeformerDataset's keys
is accepted too). draw() draws one file's parameters from a numpy Generator seeded by (--degrade_seed, crc32 of the file's input-relative
path), so a file's LQ image does not depend on the batch size, the worker count or the rank that meets it. The blur kernel is a float64
restatement of utils/degradation.py:17-110 (sigma_matrix2, mesh_grid, pdf2, bivariate_Gaussian); the noise field is drawn on the host and
travels with the image (at most a quarter of its pixels with the recipes' downsample ranges).
"""
import ctypes as C
import json
import math
import zlib
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib as L

NORMS = {"none": L.DEGRADE_NORM_NONE, "max": L.DEGRADE_NORM_MAX}
KERNELS = ("iso", "aniso")
# tools/lq.py:30-45; its last line divides by the image's maximum ("max"), which brightens every image whose LQ form has no white pixel - the
# default keeps the values (dataset/codeformer.py does), `"norm": "max"` in a recipe file gives that tool's bytes.
LQ_RECIPE = {"blur_kernel_size": 41, "kernel_list": ["iso", "aniso"], "kernel_prob": [0.5, 0.5], "blur_sigma": [0.1, 10],
             "downsample_range": [2, 4], "noise_range": [0, 20], "jpeg_range": [60, 100], "norm": "none"}
CONFLICTS = ("show_lq", "use_center_crop", "shard_tiles")   # the flags that switch the device input route off


class DegradeError(ValueError):
    pass


class Params(NamedTuple):
    """One image's record: what ir_degrade takes, plus what was drawn."""
    kernel: np.ndarray            # float64 [K][K]
    lh: int
    lw: int
    sigma: float                  # of the noise, in units of 1 / 255
    q: int                        # JPEG quality, 0: no JPEG step
    noise: Optional[np.ndarray]   # float32 [lh][lw][3] standard normal, None: no noise step
    norm: int                     # L.DEGRADE_NORM_*
    scale: float = 0.0
    kind: str = ""


def load_recipe(spec) -> dict:
    """`lq`, a dict, or the path of a JSON file with CodeformerDataset's keys (missing ones take LQ_RECIPE's values)."""
    if isinstance(spec, dict):
        rec = {**LQ_RECIPE, **spec}
    elif spec in (None, True, "lq"):
        rec = dict(LQ_RECIPE)
    else:
        with open(spec) as f:
            rec = {**LQ_RECIPE, **json.load(f)}
    unknown = sorted(set(rec) - set(LQ_RECIPE))
    if unknown:
        raise DegradeError(f"degrade recipe: unknown keys {unknown} (known: {sorted(LQ_RECIPE)})")
    for kind in rec["kernel_list"]:
        if kind not in KERNELS:
            raise DegradeError(f"degrade recipe: kernel type `{kind}` is not supported (only {', '.join(KERNELS)})")
    if len(rec["kernel_list"]) == 0 or len(rec["kernel_prob"]) != len(rec["kernel_list"]) or min(rec["kernel_prob"]) < 0 or sum(rec["kernel_prob"]) <= 0:
        raise DegradeError("degrade recipe: kernel_prob needs one non-negative weight per kernel type")
    K = rec["blur_kernel_size"]
    if not isinstance(K, int) or K < 1 or K % 2 == 0 or K > L.DEGRADE_MAX_KSIZE:
        raise DegradeError(f"degrade recipe: blur_kernel_size must be odd and within 1 .. {L.DEGRADE_MAX_KSIZE}")
    if rec["norm"] not in NORMS:
        raise DegradeError(f"degrade recipe: norm `{rec['norm']}` (known: {', '.join(NORMS)})")
    for key, lo, hi in (("blur_sigma", 1e-6, math.inf), ("downsample_range", 1.0, math.inf), ("noise_range", 0.0, math.inf), ("jpeg_range", 1.0, 101.0)):
        r = rec[key]
        if r is None and key in ("noise_range", "jpeg_range"):
            continue
        if r is None or len(r) != 2 or not lo <= r[0] <= r[1] <= hi:
            raise DegradeError(f"degrade recipe: {key} must be [low, high] within {lo} .. {hi}")
    return rec


def check_flags(args) -> None:
    """--degrade runs on the device input route of --resize gpu; refuse the flags that switch that route off, by name."""
    for flag in CONFLICTS:
        if getattr(args, flag, None):
            raise DegradeError(f"--degrade makes the LQ images on the device and cannot be combined with --{flag}")


def bivariate_gaussian(K: int, sig_x: float, sig_y: float, theta: float, isotropic: bool) -> np.ndarray:
    """utils/degradation.py:bivariate_Gaussian in float64: exp(-0.5 g^T Sigma^-1 g) on the grid -K//2+1 .. K//2, divided by its sum."""
    if isotropic:
        sigma = np.array([[sig_x ** 2, 0], [0, sig_x ** 2]])
    else:
        d = np.array([[sig_x ** 2, 0], [0, sig_y ** 2]])
        u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        sigma = np.dot(u, np.dot(d, u.T))
    ax = np.arange(-K // 2 + 1., K // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    grid = np.hstack((xx.reshape((K * K, 1)), yy.reshape(K * K, 1))).reshape(K, K, 2)
    kernel = np.exp(-0.5 * np.sum(np.dot(grid, np.linalg.inv(sigma)) * grid, 2))
    return kernel / np.sum(kernel)


def delta_kernel(K: int = 1) -> np.ndarray:
    k = np.zeros((K, K), dtype=np.float64)
    k[K // 2, K // 2] = 1.0
    return k


def file_rng(seed: int, relpath: str) -> np.random.Generator:
    return np.random.default_rng([int(seed) & 0xFFFFFFFF, zlib.crc32(str(relpath).replace("\\", "/").encode("utf-8"))])


def draw(recipe: dict, relpath: str, h: int, w: int, seed: int = 231) -> Params:
    """The parameters of the file at `relpath` (relative to the input folder), an h x w image, in CodeformerDataset's order of draws: kernel
    type, sigma_x (sigma_y and the rotation for `aniso`), the downsample scale, the noise sigma and field, the JPEG quality."""
    rng = file_rng(seed, relpath)
    K = recipe["blur_kernel_size"]
    if min(h, w) < K // 2 + 1:
        raise DegradeError(f"{relpath}: a {w} x {h} image is too small for a {K} x {K} blur")
    prob = np.asarray(recipe["kernel_prob"], dtype=np.float64)
    kind = recipe["kernel_list"][int(rng.choice(len(prob), p=prob / prob.sum()))]
    lo, hi = recipe["blur_sigma"]
    sig_x = rng.uniform(lo, hi)
    if kind == "aniso":
        sig_y, theta = rng.uniform(lo, hi), rng.uniform(-math.pi, math.pi)
    else:
        sig_y, theta = sig_x, 0.0
    kernel = bivariate_gaussian(K, sig_x, sig_y, theta, kind == "iso")
    scale = rng.uniform(*recipe["downsample_range"])
    lh, lw = int(h // scale), int(w // scale)
    if min(lh, lw) < L.DEGRADE_MIN_LOW:
        raise DegradeError(f"{relpath}: a {w} x {h} image downsampled by {scale:.2f} is below {L.DEGRADE_MIN_LOW} pixels on an edge")
    sigma, noise = 0.0, None
    if recipe["noise_range"] is not None:
        sigma = rng.uniform(*recipe["noise_range"])
        noise = rng.standard_normal((lh, lw, 3), dtype=np.float32)
    q = 0
    if recipe["jpeg_range"] is not None:
        q = min(int(rng.uniform(*recipe["jpeg_range"])), 100)
    return Params(kernel, lh, lw, float(sigma), q, noise, NORMS[recipe["norm"]], float(scale), kind)


def check_params(p: Params, h: int, w: int) -> None:
    """What ir_degrade refuses, with a message, before anything is staged."""
    k = np.asarray(p.kernel)
    K = k.shape[0]
    if k.ndim != 2 or k.shape != (K, K) or K % 2 == 0 or K > L.DEGRADE_MAX_KSIZE or k.dtype != np.float64:
        raise DegradeError(f"degrade: the blur kernel must be float64 K x K with K odd and at most {L.DEGRADE_MAX_KSIZE}")
    if min(h, w) < K // 2 + 1:
        raise DegradeError(f"degrade: a {w} x {h} image is too small for a {K} x {K} blur")
    if not (L.DEGRADE_MIN_LOW <= p.lh <= h and L.DEGRADE_MIN_LOW <= p.lw <= w):
        raise DegradeError(f"degrade: low-resolution size {p.lw} x {p.lh} outside {L.DEGRADE_MIN_LOW} .. {w} x {h}")
    if not 0 <= p.q <= 100:
        raise DegradeError(f"degrade: JPEG quality {p.q} outside 0 .. 100")
    if p.noise is not None and (p.noise.shape != (p.lh, p.lw, 3) or p.noise.dtype != np.float32):
        raise DegradeError("degrade: the noise field must be float32 [lh][lw][3]")
    if p.norm not in NORMS.values():
        raise DegradeError(f"degrade: unknown norm {p.norm}")


def extra_bytes(p: Params) -> int:
    """Bytes of the kernel and the noise field in a staging buffer (each at a 256-byte boundary)."""
    return ((p.kernel.nbytes + 255) & ~255) + (((p.noise.nbytes + 255) & ~255) if p.noise is not None else 0)


def pack_extras(p: Params, host: np.ndarray, at: int):
    """Copy the kernel and the noise field into the byte buffer `host` from offset `at` -> (kernel offset, noise offset or None, end)."""
    k_at = at
    host[at:at + p.kernel.nbytes] = np.ascontiguousarray(p.kernel).view(np.uint8).reshape(-1)
    at += (p.kernel.nbytes + 255) & ~255
    n_at = None
    if p.noise is not None:
        n_at = at
        host[at:at + p.noise.nbytes] = np.ascontiguousarray(p.noise).view(np.uint8).reshape(-1)
        at += (p.noise.nbytes + 255) & ~255
    return k_at, n_at, at


def record(p: Params, kernel_ptr: int, noise_ptr: Optional[int]) -> L.DegradeParams:
    return L.DegradeParams(kernel_ptr, noise_ptr if p.noise is not None else None, p.kernel.shape[0], p.lh, p.lw, p.q, p.norm, float(np.float32(p.sigma)))


def ws_bytes(h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_DEGRADE, 1, h, w, 0, 0, 0))


def launch(ctx, src: int, dst: int, rows: int, pitch: int, h: int, w: int, records: Sequence[L.DegradeParams], jpeg: int = 0) -> None:
    """ir_degrade on the current stream for len(records) images at src -> dst (device addresses). The scratch is the context's workspace."""
    need = ws_bytes(h, w)
    ws = ctx.workspace(need + 256)
    base = (ws.data_ptr() + 255) & ~255
    arr = (L.DegradeParams * len(records))(*records)
    ctx.check(ctx.lib.ir_degrade(ctx.h, ctx.stream(), C.c_void_p(src), rows, pitch, len(records), h, w, arr, C.c_void_p(dst),
                                 C.c_void_p(jpeg) if jpeg else None, C.c_void_p(base), need), "ir_degrade")


def degrade(ctx, imgs: Sequence[np.ndarray], params: Sequence[Params], with_jpeg: bool = False):
    """The LQ images of equal-sized HWC uint8 RGB arrays, one Params each, made on the device and downloaded (a synchronous convenience for
    tools and tests; the pipeline stages through resample.ResizeSlot). with_jpeg: also every image's bytes behind the JPEG step (None for q = 0)."""
    import torch
    imgs = [np.ascontiguousarray(a) for a in imgs]
    n, (h, w) = len(imgs), imgs[0].shape[:2]
    if n == 0 or len(params) != n or any(a.shape != (h, w, 3) or a.dtype != np.uint8 for a in imgs):
        raise DegradeError("degrade: equal-sized HWC uint8 RGB images and one record each")
    for p in params:
        check_params(p, h, w)
    img_bytes = n * h * w * 3
    total = ((img_bytes + 255) & ~255) + sum(extra_bytes(p) for p in params)
    host = np.empty(total, dtype=np.uint8)
    host[:img_bytes] = np.stack(imgs).reshape(-1)
    at, offs = (img_bytes + 255) & ~255, []
    for p in params:
        k_at, n_at, at = pack_extras(p, host, at)
        offs.append((k_at, n_at))
    dev = torch.from_numpy(host).to(ctx.device)
    out = torch.zeros(img_bytes, dtype=torch.uint8, device=ctx.device)
    mid = torch.zeros(img_bytes, dtype=torch.uint8, device=ctx.device) if with_jpeg else None
    recs = [record(p, dev.data_ptr() + k_at, dev.data_ptr() + n_at if n_at is not None else None) for p, (k_at, n_at) in zip(params, offs)]
    launch(ctx, dev.data_ptr(), out.data_ptr(), h, 3 * w, h, w, recs, mid.data_ptr() if with_jpeg else 0)
    torch.cuda.current_stream(ctx.device).synchronize()
    lq = out.cpu().numpy().reshape(n, h, w, 3)
    res = [lq[i].copy() for i in range(n)]
    if not with_jpeg:
        return res
    m = mid.cpu().numpy().reshape(n, h * w * 3)
    return res, [m[i, :p.lh * p.lw * 3].reshape(p.lh, p.lw, 3).copy() if p.q else None for i, p in enumerate(params)]
