"""Low-quality inputs synthesised from ground truth (ir_degrade, csrc/degrade.hip): the host side. The reference makes its LQ sets with
tools/lq.py, the first-order chain of dataset/codeformer.py:CodeformerDataset.__getitem__ (:140-163) - blur, bilinear downsample, noise, JPEG,
bilinear resize back - with OpenCV and a second folder of files; here the ground truth goes to the device and the LQ image is made there
(tools/degrade_folder.py is the definition, in numpy).

A recipe holds the ranges the parameters are drawn from (LQ_RECIPE: the constants of tools/lq.py; a JSON file with CodeformerDataset's keys
is accepted too). draw() draws one file's parameters from a numpy Generator seeded by (--degrade_seed, crc32 of the file's input-relative
path), so a file's LQ image does not depend on the batch size, the worker count or the rank that meets it. The blur kernel is a float64
restatement of utils/degradation.py:17-110 (sigma_matrix2, mesh_grid, pdf2, bivariate_Gaussian); the noise field is drawn on the host and
travels with the image (at most a quarter of its pixels with the recipes' downsample ranges).

`realesrgan` is the second-order recipe the reference validates general super-resolution with (configs/general_deg_realesrgan_val.yaml,
dataset/realesrgan.py, dataset/batch_transform.py:RealESRGANBatchTransform): REALESRGAN_RECIPE restates its parameters, draw_chain() draws one
file's CHAIN of ops (ChainParams: filters, resizes, Gaussian or Poisson noise, DiffJPEG, in the reference's order of decisions) from the same
per-file generator, and ir_degrade_chain (csrc/degrade_chain.hip) runs it; tools/degrade_folder.py:degrade_chain_model is the definition.
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
    """`lq`, `realesrgan`, a dict, or the path of a JSON file with CodeformerDataset's keys (missing ones take LQ_RECIPE's values); a dict or
    file with `"chain": "realesrgan"` holds REALESRGAN_RECIPE's keys instead."""
    if spec == "realesrgan":
        spec = {"chain": "realesrgan"}
    elif not isinstance(spec, dict) and spec not in (None, True, "lq"):
        with open(spec) as f:
            spec = json.load(f)
    if isinstance(spec, dict) and "chain" in spec:
        return _load_chain_recipe(spec)
    if isinstance(spec, dict):
        rec = {**LQ_RECIPE, **spec}
    else:
        rec = dict(LQ_RECIPE)
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
    crop_on_gpu = getattr(args, "center_crop", "host") == "gpu"   # --center_crop gpu: the crop is made on that route too, and is what is degraded
    for flag in CONFLICTS:
        if getattr(args, flag, None) and not (flag == "use_center_crop" and crop_on_gpu):
            raise DegradeError(f"--degrade makes the LQ images on the device and cannot be combined with --{flag}"
                               + (" (or give --center_crop gpu)" if flag == "use_center_crop" else ""))


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


def draw(recipe: dict, relpath: str, h: int, w: int, seed: int = 231):
    """The parameters of the file at `relpath` (relative to the input folder), an h x w image, in CodeformerDataset's order of draws: kernel
    type, sigma_x (sigma_y and the rotation for `aniso`), the downsample scale, the noise sigma and field, the JPEG quality. A recipe of
    the `realesrgan` kind gives draw_chain()'s ChainParams."""
    if recipe.get("chain"):
        return draw_chain(recipe, relpath, h, w, seed)
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


def check_params(p, h: int, w: int) -> None:
    """What ir_degrade (ir_degrade_chain for ChainParams) refuses, with a message, before anything is staged."""
    if isinstance(p, ChainParams):
        check_chain(p, h, w)
        return
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


def extra_bytes(p) -> int:
    """Bytes of the kernel and the noise field (of a chain's kernels and fields) in a staging buffer (each at a 256-byte boundary)."""
    if isinstance(p, ChainParams):
        return sum((a.nbytes + 255) & ~255 for a in _chain_arrays(p))
    return ((p.kernel.nbytes + 255) & ~255) + (((p.noise.nbytes + 255) & ~255) if p.noise is not None else 0)


def pack_extras(p, host: np.ndarray, at: int):
    """Copy the kernel and the noise field into the byte buffer `host` from offset `at` -> (kernel offset, noise offset or None, end); for
    ChainParams -> (the offsets of its ops' arrays, None for an op without one, None, end)."""
    if isinstance(p, ChainParams):
        offs = []
        for op in p.ops:
            a = _op_array(op)
            offs.append(None if a is None else at)
            if a is not None:
                host[at:at + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                at += (a.nbytes + 255) & ~255
        return offs, None, at
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


# ---------------------------------------------------------------- the second-order chain (ir_degrade_chain)
CHAIN_KERNELS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
CHAIN_MODES = {"area": L.CHAIN_AREA, "bilinear": L.CHAIN_BILINEAR, "bicubic": L.CHAIN_BICUBIC}
# configs/general_deg_realesrgan_val.yaml: the dataset's kernel settings and the batch transform's parameters in one flat dict (the file list, the
# crop, the flips and the training queue are not degradation parameters); tests/golden/realesrgan_val.json is read from the yaml itself.
REALESRGAN_RECIPE = {
    "chain": "realesrgan",
    "blur_kernel_size": 21, "kernel_list": list(CHAIN_KERNELS), "kernel_prob": [0.45, 0.25, 0.12, 0.03, 0.12, 0.03], "sinc_prob": 0.1,
    "blur_sigma": [0.2, 3], "betag_range": [0.5, 4], "betap_range": [1, 2],
    "blur_kernel_size2": 21, "kernel_list2": list(CHAIN_KERNELS), "kernel_prob2": [0.45, 0.25, 0.12, 0.03, 0.12, 0.03], "sinc_prob2": 0.1,
    "blur_sigma2": [0.2, 1.5], "betag_range2": [0.5, 4], "betap_range2": [1, 2], "final_sinc_prob": 0.8,
    "use_sharpener": False, "resize_hq": False,
    "resize_prob": [0.2, 0.7, 0.1], "resize_range": [0.15, 1.5], "gaussian_noise_prob": 0.5, "noise_range": [1, 30],
    "poisson_scale_range": [0.05, 3], "gray_noise_prob": 0.4, "jpeg_range": [30, 95],
    "stage2_scale": 4, "second_blur_prob": 0.8, "resize_prob2": [0.3, 0.4, 0.3], "resize_range2": [0.3, 1.2], "gaussian_noise_prob2": 0.5,
    "noise_range2": [1, 25], "poisson_scale_range2": [0.05, 2.5], "gray_noise_prob2": 0.4, "jpeg_range2": [30, 95]}


class ChainParams(NamedTuple):
    """One image's chain: the ops in tools/degrade_folder.py's form - (CHAIN_FILTER, kernel float64 [K][K]), (CHAIN_RESIZE, mode, oh, ow,
    scale factor or 0), (CHAIN_GAUSS, field float32, sigma, gray), (CHAIN_POISSON, u float64, scale, gray), (CHAIN_DIFFJPEG, quality) - and
    what was drawn, by name."""
    ops: tuple
    info: dict = {}

    def describe(self) -> str:
        names = {L.CHAIN_FILTER: "filter", L.CHAIN_RESIZE: "resize", L.CHAIN_GAUSS: "gauss", L.CHAIN_POISSON: "poisson", L.CHAIN_DIFFJPEG: "jpeg"}
        out = []
        for op in self.ops:
            if op[0] == L.CHAIN_RESIZE:
                out.append(f"{[k for k, v in CHAIN_MODES.items() if v == op[1]][0]} {op[3]} x {op[2]}")
            elif op[0] == L.CHAIN_FILTER:
                out.append("filter")
            elif op[0] == L.CHAIN_DIFFJPEG:
                out.append(f"jpeg {float(op[1]):.1f}")
            else:
                out.append(f"{'gray ' if op[3] else ''}{names[op[0]]} {float(op[2]):.2f}")
        return ", ".join(out)


def _load_chain_recipe(spec: dict) -> dict:
    if spec["chain"] != "realesrgan":
        raise DegradeError(f"degrade recipe: unknown chain `{spec['chain']}` (known: realesrgan)")
    rec = {**REALESRGAN_RECIPE, **spec}
    unknown = sorted(set(rec) - set(REALESRGAN_RECIPE))
    if unknown:
        raise DegradeError(f"degrade recipe: unknown keys {unknown} (known: {sorted(REALESRGAN_RECIPE)})")
    for flag in ("use_sharpener", "resize_hq"):
        if rec[flag]:
            raise DegradeError(f"degrade recipe: {flag} is outside the validation recipe and not supported")
    for sfx in ("", "2"):
        for kind in rec["kernel_list" + sfx]:
            if kind not in CHAIN_KERNELS:
                raise DegradeError(f"degrade recipe: kernel type `{kind}` is not supported (only {', '.join(CHAIN_KERNELS)})")
        prob = rec["kernel_prob" + sfx]
        if len(prob) == 0 or len(prob) != len(rec["kernel_list" + sfx]) or min(prob) < 0 or sum(prob) <= 0:
            raise DegradeError(f"degrade recipe: kernel_prob{sfx} needs one non-negative weight per kernel type")
        K = rec["blur_kernel_size" + sfx]
        if not isinstance(K, int) or K < 7 or K % 2 == 0 or K > L.CHAIN_MAX_KSIZE:
            raise DegradeError(f"degrade recipe: blur_kernel_size{sfx} must be odd and within 7 .. {L.CHAIN_MAX_KSIZE}")
        for key, lo, hi in (("blur_sigma", 1e-6, math.inf), ("betag_range", 1e-6, math.inf), ("betap_range", 1e-6, math.inf), ("resize_range", 1e-3, 8.0),
                            ("noise_range", 0.0, math.inf), ("poisson_scale_range", 0.0, math.inf), ("jpeg_range", 1.0, 100.0)):
            r = rec[key + sfx]
            if r is None or len(r) != 2 or not lo <= r[0] <= r[1] <= hi:
                raise DegradeError(f"degrade recipe: {key}{sfx} must be [low, high] within {lo} .. {hi}")
        if not rec["resize_range" + sfx][0] <= 1 <= rec["resize_range" + sfx][1]:
            raise DegradeError(f"degrade recipe: resize_range{sfx} must hold 1")
        p3 = rec["resize_prob" + sfx]
        if len(p3) != 3 or min(p3) < 0 or sum(p3) <= 0:
            raise DegradeError(f"degrade recipe: resize_prob{sfx} needs three non-negative weights (up, down, keep)")
    s2 = rec["stage2_scale"]
    s2 = [s2, s2] if isinstance(s2, (int, float)) else s2
    if len(s2) != 2 or not 1 <= s2[0] <= s2[1] <= 16:
        raise DegradeError("degrade recipe: stage2_scale must be a number or [low, high] within 1 .. 16")
    return rec


def _quadratic_form(K: int, sig_x: float, sig_y: float, theta: float, isotropic: bool) -> np.ndarray:
    """g^T Sigma^-1 g on the grid of bivariate_gaussian()."""
    if isotropic:
        sigma = np.array([[sig_x ** 2, 0], [0, sig_x ** 2]])
    else:
        d = np.array([[sig_x ** 2, 0], [0, sig_y ** 2]])
        u = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        sigma = np.dot(u, np.dot(d, u.T))
    ax = np.arange(-K // 2 + 1., K // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    grid = np.hstack((xx.reshape((K * K, 1)), yy.reshape(K * K, 1))).reshape(K, K, 2)
    return np.sum(np.dot(grid, np.linalg.inv(sigma)) * grid, 2)


def generalized_gaussian(K: int, sig_x: float, sig_y: float, theta: float, beta: float, isotropic: bool) -> np.ndarray:
    """utils/degradation.py:bivariate_generalized_Gaussian in float64: exp(-0.5 (g^T Sigma^-1 g) ** beta), divided by its sum."""
    kernel = np.exp(-0.5 * np.power(_quadratic_form(K, sig_x, sig_y, theta, isotropic), beta))
    return kernel / np.sum(kernel)


def plateau(K: int, sig_x: float, sig_y: float, theta: float, beta: float, isotropic: bool) -> np.ndarray:
    """utils/degradation.py:bivariate_plateau in float64: 1 / ((g^T Sigma^-1 g) ** beta + 1), divided by its sum."""
    kernel = np.reciprocal(np.power(_quadratic_form(K, sig_x, sig_y, theta, isotropic), beta) + 1)
    return kernel / np.sum(kernel)


def circular_lowpass_kernel(cutoff: float, K: int, pad_to: int = 0) -> np.ndarray:
    """utils/degradation.py:circular_lowpass_kernel in float64: the 2-D sinc filter cutoff J1(cutoff r) / (2 pi r), cutoff ** 2 / (4 pi) in the
    centre, divided by its sum, zero padded to pad_to. Needs scipy (special.j1)."""
    try:
        from scipy import special
    except ImportError as e:
        raise DegradeError(f"the realesrgan recipe's sinc kernels need scipy (scipy.special.j1): {e}")
    c = (K - 1) / 2
    yy, xx = np.meshgrid(np.arange(K, dtype=np.float64), np.arange(K, dtype=np.float64), indexing="ij")
    r = np.sqrt((yy - c) ** 2 + (xx - c) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        kernel = cutoff * special.j1(cutoff * r) / (2 * np.pi * r)
    kernel[(K - 1) // 2, (K - 1) // 2] = cutoff ** 2 / (4 * np.pi)
    kernel = kernel / np.sum(kernel)
    return pad_kernel(kernel, pad_to) if pad_to > K else kernel


def pad_kernel(k: np.ndarray, to: int = L.CHAIN_MAX_KSIZE) -> np.ndarray:
    pad = (to - k.shape[0]) // 2
    return np.pad(k, ((pad, pad), (pad, pad)))


def _choice(rng, weights) -> int:
    p = np.asarray(weights, dtype=np.float64)
    return int(rng.choice(len(p), p=p / p.sum()))


def mixed_kernel(rng, kinds, prob, K: int, sigma_range, betag_range, betap_range):
    """utils/degradation.py:random_mixed_kernels: the type, sigma_x, (sigma_y and the rotation for an anisotropic type), and for the generalized
    and plateau types the beta rule - a coin, then beta from [low, 1] or from [1, high]. -> (kernel, what was drawn)."""
    kind = kinds[_choice(rng, prob)]
    iso = kind.endswith("iso") and not kind.endswith("aniso")
    sig_x = rng.uniform(*sigma_range)
    sig_y, theta = (sig_x, 0.0) if iso else (rng.uniform(*sigma_range), rng.uniform(-math.pi, math.pi))
    info = {"kind": kind, "sig_x": sig_x, "sig_y": sig_y, "theta": theta}
    if kind in ("iso", "aniso"):
        return bivariate_gaussian(K, sig_x, sig_y, theta, iso), info
    lo, hi = betag_range if kind.startswith("generalized") else betap_range
    beta = rng.uniform(lo, 1) if rng.uniform() < 0.5 else rng.uniform(1, hi)
    info["beta"] = beta
    return (generalized_gaussian if kind.startswith("generalized") else plateau)(K, sig_x, sig_y, theta, beta, iso), info


def _draw_kernel(rng, rec: dict, sfx: str):
    """dataset/realesrgan.py:129-151: the size from 7, 9 .. blur_kernel_size, the sinc coin, then the sinc's cutoff or a mixed kernel."""
    K = int(rng.choice(np.arange(7, rec["blur_kernel_size" + sfx] + 1, 2)))
    if rng.uniform() < rec["sinc_prob" + sfx]:
        omega = rng.uniform(np.pi / 3 if K < 13 else np.pi / 5, np.pi)
        k, info = circular_lowpass_kernel(omega, K), {"kind": "sinc", "omega": omega}
    else:
        k, info = mixed_kernel(rng, rec["kernel_list" + sfx], rec["kernel_prob" + sfx], K, rec["blur_sigma" + sfx], rec["betag_range" + sfx],
                               rec["betap_range" + sfx])
    info["size"] = K
    return pad_kernel(k), info


def _draw_resize(rng, rec: dict, sfx: str):
    updown = _choice(rng, rec["resize_prob" + sfx])
    lo, hi = rec["resize_range" + sfx]
    scale = rng.uniform(1, hi) if updown == 0 else (rng.uniform(lo, 1) if updown == 1 else 1.0)
    return float(scale), int(rng.integers(3))


def _draw_noise(rng, rec: dict, sfx: str, h: int, w: int):
    if rng.uniform() < rec["gaussian_noise_prob" + sfx]:
        sigma = rng.uniform(*rec["noise_range" + sfx])
        gray = bool(rng.uniform() < rec["gray_noise_prob" + sfx])
        return (L.CHAIN_GAUSS, rng.standard_normal((h, w) if gray else (h, w, 3), dtype=np.float32), float(np.float32(sigma)), gray)
    scale = rng.uniform(*rec["poisson_scale_range" + sfx])
    gray = bool(rng.uniform() < rec["gray_noise_prob" + sfx])
    return (L.CHAIN_POISSON, rng.random((h, w) if gray else (h, w, 3)), float(np.float32(scale)), gray)


def draw_chain(recipe: dict, relpath: str, h: int, w: int, seed: int = 231) -> ChainParams:
    """The chain of the file at `relpath`, an h x w image, from file_rng in RealESRGANDataset's and RealESRGANBatchTransform's order of
    decisions: kernel 1, kernel 2, the final sinc; stage 1 - up / down / keep with its scale, the mode, Gaussian or Poisson noise with its
    level and gray flag (and the field, which this project draws on the host), the JPEG quality; the second-blur coin; stage 2 - its resize
    and noise; the order coin (resize + sinc then JPEG, or JPEG then resize + sinc) with that mode and quality; bicubic back to h x w when
    stage2_scale is not 1. A final sinc that came out as the pulse is no op at all (with fp64 sums the filter would change nothing)."""
    rng = file_rng(seed, relpath)
    k1, i1 = _draw_kernel(rng, recipe, "")
    k2, i2 = _draw_kernel(rng, recipe, "2")
    sinc, i3 = None, {"kind": "pulse"}
    if rng.uniform() < recipe["final_sinc_prob"]:
        K = int(rng.choice(np.arange(7, L.CHAIN_MAX_KSIZE + 1, 2)))
        omega = rng.uniform(np.pi / 3, np.pi)
        sinc, i3 = circular_lowpass_kernel(omega, K, L.CHAIN_MAX_KSIZE), {"kind": "sinc", "omega": omega, "size": K}
    ops = [(L.CHAIN_FILTER, k1)]
    scale, mode = _draw_resize(rng, recipe, "")
    ch, cw = int(math.floor(h * scale)), int(math.floor(w * scale))
    ops.append((L.CHAIN_RESIZE, mode, ch, cw, scale))
    if min(ch, cw) >= 1:
        ops.append(_draw_noise(rng, recipe, "", ch, cw))
    ops.append((L.CHAIN_DIFFJPEG, float(np.float32(rng.uniform(*recipe["jpeg_range"])))))
    if rng.uniform() < recipe["second_blur_prob"]:
        ops.append((L.CHAIN_FILTER, k2))
    s2 = recipe["stage2_scale"]
    s2 = float(s2) if isinstance(s2, (int, float)) else rng.uniform(*s2)
    s2h, s2w = int(h / s2), int(w / s2)
    scale2, mode2 = _draw_resize(rng, recipe, "2")
    ch, cw = int(s2h * scale2), int(s2w * scale2)
    ops.append((L.CHAIN_RESIZE, mode2, ch, cw, 0.0))
    if min(ch, cw) >= 1:
        ops.append(_draw_noise(rng, recipe, "2", ch, cw))
    back_first = bool(rng.uniform() < 0.5)
    if back_first:
        ops.append((L.CHAIN_RESIZE, int(rng.integers(3)), s2h, s2w, 0.0))
        if sinc is not None:
            ops.append((L.CHAIN_FILTER, sinc))
        ops.append((L.CHAIN_DIFFJPEG, float(np.float32(rng.uniform(*recipe["jpeg_range2"])))))
    else:
        ops.append((L.CHAIN_DIFFJPEG, float(np.float32(rng.uniform(*recipe["jpeg_range2"])))))
        ops.append((L.CHAIN_RESIZE, int(rng.integers(3)), s2h, s2w, 0.0))
        if sinc is not None:
            ops.append((L.CHAIN_FILTER, sinc))
    if s2 != 1:
        ops.append((L.CHAIN_RESIZE, L.CHAIN_BICUBIC, h, w, 0.0))
    p = ChainParams(tuple(ops), {"kernel1": i1, "kernel2": i2, "final_sinc": i3, "stage2_scale": s2, "back_first": back_first})
    try:
        check_chain(p, h, w)
    except DegradeError as e:
        raise DegradeError(f"{relpath}: {e}")
    return p


def _op_array(op) -> Optional[np.ndarray]:
    return op[1] if op[0] in (L.CHAIN_FILTER, L.CHAIN_GAUSS, L.CHAIN_POISSON) else None


def _chain_arrays(p: ChainParams):
    return [a for a in map(_op_array, p.ops) if a is not None]


def check_chain(p: ChainParams, h: int, w: int):
    """What ir_degrade_chain refuses, with a message -> the largest height and the largest width among the chain's images."""
    if not 0 <= len(p.ops) <= L.CHAIN_MAX_OPS:
        raise DegradeError(f"degrade chain: at most {L.CHAIN_MAX_OPS} ops")
    ch, cw, mh, mw = h, w, h, w
    for i, op in enumerate(p.ops):
        kind = op[0]
        if kind == L.CHAIN_FILTER:
            k = np.asarray(op[1])
            K = k.shape[0]
            if k.ndim != 2 or k.shape != (K, K) or K % 2 == 0 or K > L.CHAIN_MAX_KSIZE or k.dtype != np.float64:
                raise DegradeError(f"degrade chain: op {i}: the filter must be float64 K x K with K odd and at most {L.CHAIN_MAX_KSIZE}")
            if min(ch, cw) < K // 2 + 1:
                raise DegradeError(f"degrade chain: op {i}: a {cw} x {ch} image is too small for a {K} x {K} filter (a {w} x {h} file; the reflection "
                                   f"needs {K // 2 + 1} pixels)")
        elif kind == L.CHAIN_RESIZE:
            _, mode, oh, ow, scale = op
            if mode not in CHAIN_MODES.values():
                raise DegradeError(f"degrade chain: op {i}: unknown resize mode {mode}")
            if scale and (oh, ow) != (int(math.floor(ch * scale)), int(math.floor(cw * scale))):
                raise DegradeError(f"degrade chain: op {i}: with scale factor {scale} the output is floor(in * scale), not {ow} x {oh}")
            if not (1 <= oh <= L.CHAIN_MAX_SIDE and 1 <= ow <= L.CHAIN_MAX_SIDE) or scale < 0:
                raise DegradeError(f"degrade chain: op {i}: output size {ow} x {oh} outside 1 .. {L.CHAIN_MAX_SIDE}")
            ch, cw = oh, ow
            mh, mw = max(mh, ch), max(mw, cw)
        elif kind in (L.CHAIN_GAUSS, L.CHAIN_POISSON):
            a, gray = np.asarray(op[1]), bool(op[3])
            want = np.float32 if kind == L.CHAIN_GAUSS else np.float64
            if a.shape != ((ch, cw) if gray else (ch, cw, 3)) or a.dtype != want:
                raise DegradeError(f"degrade chain: op {i}: the field must be {np.dtype(want).name} [{ch}][{cw}]{'' if gray else '[3]'}")
            if not op[2] >= 0:
                raise DegradeError(f"degrade chain: op {i}: a negative noise level")
        elif kind == L.CHAIN_DIFFJPEG:
            if not 1 <= op[1] <= 100:
                raise DegradeError(f"degrade chain: op {i}: JPEG quality {op[1]} outside 1 .. 100")
        else:
            raise DegradeError(f"degrade chain: op {i}: unknown kind {kind}")
    if (ch, cw) != (h, w):
        raise DegradeError(f"degrade chain: the chain ends at {cw} x {ch}, not at the image's {w} x {h}")
    return mh, mw


def jpeg_factor(quality) -> np.float32:
    """diffjpeg.py:quality_to_factor on a float32 tensor element (tools/degrade_folder.py:jpeg_factor)."""
    q = np.float32(quality)
    return (np.float32(5000.0) / q if q < 50 else np.float32(200.0) - q * np.float32(2.0)) / np.float32(100.0)


def chain_tables() -> np.ndarray:
    """float64: exp(-lambda) [9][256] of the Poisson inversion, then the DiffJPEG basis [64][64] with the module's scale [64] and alpha [64]
    behind it - tools/degrade_folder.py's poisson_exp_table, dct_basis, DCT_SCALE and IDCT_ALPHA, computed by numpy once and handed to every call."""
    r = np.arange(256, dtype=np.float32) / np.float32(255.0)
    table = np.stack([np.exp(-(r * np.float32(1 << j)).astype(np.float64)) for j in range(9)])
    i = np.arange(8)
    c = np.cos((2 * i[:, None] + 1) * i[None, :] * np.pi / 16)
    basis = (c[:, None, :, None] * c[None, :, None, :]).astype(np.float32).astype(np.float64).reshape(64, 64)
    alpha = np.array([1.0 / np.sqrt(2)] + [1.0] * 7)
    scale = (np.outer(alpha, alpha) * 0.25).astype(np.float32).astype(np.float64)
    return np.concatenate([table.reshape(-1), basis.reshape(-1), scale.reshape(-1), np.outer(alpha, alpha).astype(np.float32).astype(np.float64).reshape(-1)])


def _device_tables(ctx):
    import torch
    t = getattr(ctx, "_chain_tables", None)
    if t is None:
        t = ctx._chain_tables = torch.from_numpy(chain_tables()).to(ctx.device)
    return t


def chain_record(p: ChainParams, base: int, offs, tables: int, tap: int = -1) -> L.Chain:
    """The ir_chain of one image: its arrays lie at base + offs[i] (pack_extras), the tables at `tables` (device addresses)."""
    rec = L.Chain()
    rec.n_ops, rec.tap, rec.exp_table, rec.dct_basis = len(p.ops), tap, tables, tables + 9 * 256 * 8
    for i, (op, o) in enumerate(zip(p.ops, offs)):
        r = rec.ops[i]
        r.kind, r.data = op[0], (base + o if o is not None else None)
        if op[0] == L.CHAIN_FILTER:
            r.a = op[1].shape[0]
        elif op[0] == L.CHAIN_RESIZE:
            r.a, r.b, r.c, r.s = op[1], op[2], op[3], float(op[4])
        elif op[0] in (L.CHAIN_GAUSS, L.CHAIN_POISSON):
            r.a, r.s = int(bool(op[3])), float(np.float32(op[2]))
        else:
            r.s = float(jpeg_factor(op[1]))
    return rec


def chain_ws_bytes(h: int, w: int, mh: int, mw: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 1, h, w, mh, mw, 0))


def launch_chain(ctx, src: int, dst: int, rows: int, pitch: int, h: int, w: int, records: Sequence[L.Chain], sizes, tap: int = 0) -> None:
    """ir_degrade_chain on the current stream for len(records) images at src -> dst (device addresses); sizes: check_chain()'s largest
    height and width over the records. The scratch is the context's workspace."""
    need = chain_ws_bytes(h, w, sizes[0], sizes[1])
    ws = ctx.workspace(need + 256)
    base = (ws.data_ptr() + 255) & ~255
    arr = (L.Chain * len(records))(*records)
    ctx.check(ctx.lib.ir_degrade_chain(ctx.h, ctx.stream(), C.c_void_p(src), rows, pitch, len(records), h, w, arr, C.c_void_p(dst),
                                       C.c_void_p(tap) if tap else None, C.c_void_p(base), need), "ir_degrade_chain")


def launch_chain_params(ctx, p: ChainParams, src: int, dst: int, h: int, w: int, base: int, offs) -> None:
    """One staged file (resample.ResizeSlot): its chain from src to dst, its arrays at base + offs."""
    launch_chain(ctx, src, dst, h, 3 * w, h, w, [chain_record(p, base, offs, _device_tables(ctx).data_ptr())], check_chain(p, h, w))


def degrade_chain(ctx, imgs: Sequence[np.ndarray], params: Sequence[ChainParams], taps: Optional[Sequence[int]] = None):
    """The LQ images of equal-sized HWC uint8 RGB arrays, one ChainParams each, made on the device and downloaded (a synchronous convenience
    for tools and tests). taps: per image the index of the op whose float32 image is returned as well (-1: none) -> (images, tap images)."""
    import torch
    imgs = [np.ascontiguousarray(a) for a in imgs]
    n, (h, w) = len(imgs), imgs[0].shape[:2]
    if n == 0 or len(params) != n or any(a.shape != (h, w, 3) or a.dtype != np.uint8 for a in imgs):
        raise DegradeError("degrade: equal-sized HWC uint8 RGB images and one chain each")
    sizes = [check_chain(p, h, w) for p in params]
    mh, mw = max(s[0] for s in sizes), max(s[1] for s in sizes)
    img_bytes = n * h * w * 3
    total = ((img_bytes + 255) & ~255) + sum(extra_bytes(p) for p in params)
    host = np.zeros(total, dtype=np.uint8)
    host[:img_bytes] = np.stack(imgs).reshape(-1)
    at, offs = (img_bytes + 255) & ~255, []
    for p in params:
        o, _, at = pack_extras(p, host, at)
        offs.append(o)
    dev = torch.from_numpy(host).to(ctx.device)
    out = torch.zeros(img_bytes, dtype=torch.uint8, device=ctx.device)
    tables = _device_tables(ctx).data_ptr()
    recs = [chain_record(p, dev.data_ptr(), o, tables, -1 if taps is None else taps[i]) for i, (p, o) in enumerate(zip(params, offs))]
    shapes = [tap_shape(p, h, w, t) for p, t in zip(params, taps)] if taps is not None else []
    tap = torch.zeros(max(1, sum(int(np.prod(s)) for s in shapes)), dtype=torch.float32, device=ctx.device) if taps is not None else None
    launch_chain(ctx, dev.data_ptr(), out.data_ptr(), h, 3 * w, h, w, recs, (mh, mw), tap.data_ptr() if tap is not None else 0)
    torch.cuda.current_stream(ctx.device).synchronize()
    lq = out.cpu().numpy().reshape(n, h, w, 3)
    res = [lq[i].copy() for i in range(n)]
    if taps is None:
        return res
    flat, at, got = tap.cpu().numpy(), 0, []
    for s in shapes:
        got.append(flat[at:at + int(np.prod(s))].reshape(s).copy() if s[0] else None)
        at += int(np.prod(s))
    return res, got


def tap_shape(p: ChainParams, h: int, w: int, tap: int):
    """The shape of the float32 image behind op `tap` ((0, 0, 3) for tap = -1): the tap images of a batch lie behind each other."""
    if tap < 0:
        return (0, 0, 3)
    for op in p.ops[:tap + 1]:
        if op[0] == L.CHAIN_RESIZE:
            h, w = op[2], op[3]
    return (h, w, 3)
