#!/usr/bin/env python3
"""FID of a folder of results against a folder of references, or against the saved statistics of a clean set.

This file is the definition of the device call ir_fid_features (csrc/fid.hip): a restatement in torch (fp32 or fp64) of the Inception-v3 that
pytorch-fid evaluates (`InceptionV3(output_blocks=[3])`, the pooled 2048 vector), of the two ways its input is made, and of the Frechet distance.
It is restated from the published model; parity with pytorch-fid, pyiqa and clean-fid themselves is unpinned (docs/parity.md, "FID").

Network: every conv is conv without bias -> BatchNorm (eval, eps 1e-3) -> ReLU; state-dict names are torchvision's. FID's three departures from
torchvision's Inception-v3: the average pools of the A, C and first E blocks exclude the padding from their divisor, the last block (Mixed_7c)
pools with max, and the network ends at the pooled vector (`fc.*` and `AuxLogits.*` are ignored).

Input, `clean` (pyiqa's `fid`, clean-fid): every colour plane is resized to 299 x 299 as a float32 image with Pillow's BICUBIC (antialiased; the
coefficients in double, each pass accumulating in double and storing float32), clipped to [0, 255], then (v - 128) / 128. `legacy` (pytorch-fid):
v / 255, torch's bilinear interpolation without antialiasing, then 2 x - 1.

Distance, fp64: d^2 = |mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr (s1 s2)^1/2 with the last trace as the sum of sqrt(max(l, 0)) over the eigenvalues l of
s1^1/2 s2 s1^1/2 (two numpy.linalg.eigh): real, no scipy, and defined for singular covariances.

  evaluate_fid.py --model pt_inception.pth RESULTS REFERENCE
  evaluate_fid.py --model pt_inception.pth RESULTS --stats clean_set.npz
  evaluate_fid.py --features fid_features.rank0.npz fid_features.rank1.npz [--stats clean_set.npz]
"""
import argparse
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SIZE = 299
DIM = 2048
EPS = 1e-3


# ---------------------------------------------------------------- the network's table
def _a(name, cin, pf):
    return [(f"{name}.branch1x1", cin, 64, 1, 1, 1, 0, 0), (f"{name}.branch5x5_1", cin, 48, 1, 1, 1, 0, 0), (f"{name}.branch5x5_2", 48, 64, 5, 5, 1, 2, 2),
            (f"{name}.branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0), (f"{name}.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), (f"{name}.branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
            (f"{name}.branch_pool", cin, pf, 1, 1, 1, 0, 0)]


def _c(name, c7):
    return [(f"{name}.branch1x1", 768, 192, 1, 1, 1, 0, 0),
            (f"{name}.branch7x7_1", 768, c7, 1, 1, 1, 0, 0), (f"{name}.branch7x7_2", c7, c7, 1, 7, 1, 0, 3), (f"{name}.branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
            (f"{name}.branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0), (f"{name}.branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0), (f"{name}.branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3),
            (f"{name}.branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0), (f"{name}.branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3),
            (f"{name}.branch_pool", 768, 192, 1, 1, 1, 0, 0)]


def _e(name, cin):
    return [(f"{name}.branch1x1", cin, 320, 1, 1, 1, 0, 0),
            (f"{name}.branch3x3_1", cin, 384, 1, 1, 1, 0, 0), (f"{name}.branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), (f"{name}.branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
            (f"{name}.branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0), (f"{name}.branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
            (f"{name}.branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), (f"{name}.branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
            (f"{name}.branch_pool", cin, 192, 1, 1, 1, 0, 0)]


# (torchvision name, cin, cout, kh, kw, stride, pad_h, pad_w) of the 94 convolutions, in the order ir_fid_configure binds them
CONVS: List[Tuple[str, int, int, int, int, int, int, int]] = (
    [("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0), ("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0), ("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1),
     ("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0), ("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0)]
    + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64)
    + [("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0), ("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0), ("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1),
       ("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0)]
    + _c("Mixed_6b", 128) + _c("Mixed_6c", 160) + _c("Mixed_6d", 160) + _c("Mixed_6e", 192)
    + [("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0),
       ("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0), ("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3), ("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0),
       ("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0)]
    + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
# the maps whose per-channel spatial means ir_fid_features can return, and their widths
BLOCKS = ["Conv2d_2b_3x3", "Conv2d_4a_3x3", "Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b",
          "Mixed_7c"]
BLOCK_WIDTH = [64, 192, 256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
BN_PARTS = (("bn_w", "bn.weight"), ("bn_b", "bn.bias"), ("bn_mean", "bn.running_mean"), ("bn_var", "bn.running_var"))


def macs_per_image() -> int:
    """Multiply-accumulates of the 94 convolutions for one 299 x 299 image."""
    size = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71, "Mixed_5": 35, "Mixed_6": 17, "Mixed_7": 8}
    total = 0
    for name, cin, cout, kh, kw, stride, _, _ in CONVS:
        out = size[name] if name in size else size[name[:7]]
        if name in ("Mixed_6a.branch3x3", "Mixed_6a.branch3x3dbl_3"):
            out = 17
        elif name.startswith("Mixed_6a"):
            out = 35
        elif name in ("Mixed_7a.branch3x3_2", "Mixed_7a.branch7x7x3_4"):
            out = 8
        elif name.startswith("Mixed_7a"):
            out = 17
        total += out * out * cout * cin * kh * kw
    return total


def tensor_names() -> List[str]:
    """The names ir_fid_configure binds, in order."""
    return [f"fid.{name}.{p}" for name, *_ in CONVS for p in ("w", "bn_w", "bn_b", "bn_mean", "bn_var")]


def load_weights(src) -> Dict[str, "torch.Tensor"]:
    """The tensors ir_fid_configure binds (`fid.<torchvision name>.w / .bn_w / .bn_b / .bn_mean / .bn_var`, fp32) from a pytorch-fid / torchvision
    state dict (`<name>.conv.weight`, `<name>.bn.weight | bias | running_mean | running_var`; `fc.*`, `AuxLogits.*` and `num_batches_tracked` are
    ignored), from an .npz (or a dict) in ir_fid_configure's own names, or from the file of either. KeyError for a missing key, ValueError for a
    shape that is not Inception-v3's; both name the key."""
    import torch
    where = ""
    if isinstance(src, (str, os.PathLike)):
        where = f"{src}: "
        if str(src).endswith(".npz"):
            with np.load(src) as z:
                src = {k: z[k] for k in z.files}
        else:
            src = torch.load(src, map_location="cpu", weights_only=True)
            if isinstance(src, dict) and "state_dict" in src:
                src = src["state_dict"]
    own = any(str(k).startswith("fid.") for k in src)
    out = {}
    for name, cin, cout, kh, kw, _, _, _ in CONVS:
        keys = [(f"fid.{name}.w", f"{name}.conv.weight", (cout, cin, kh, kw))] + [(f"fid.{name}.{p}", f"{name}.{q}", (cout,)) for p, q in BN_PARTS]
        for mine, theirs, shape in keys:
            key = mine if own else theirs
            if key not in src:
                raise KeyError(f"{where}{key} missing")
            t = torch.as_tensor(np.asarray(src[key]) if not torch.is_tensor(src[key]) else src[key]).detach().to(torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{where}{key} has shape {tuple(t.shape)}, Inception-v3 has {shape}")
            out[mine] = t
    return out


# ---------------------------------------------------------------- the input
def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def clean_tables(size_in: int, size_out: int = SIZE, antialias: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs for BICUBIC over the whole axis: bounds [out][2] int32 (first tap, taps) and the normalised coefficients
    [out][ksize] float64 (zero behind the taps), in Pillow's order of operations."""
    scale = float(np.float32(size_in)) / size_out
    filterscale = max(scale, 1.0) if antialias else 1.0   # antialias=False: the same kernel at its own width - NOT the definition (tests)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((size_out, 2), np.int32)
    kk = np.zeros((size_out, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(size_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), size_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            kk[xx, x] = w[x] / ww if ww != 0.0 else w[x]
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clean_pass(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """Resample axis 0 of img [len][...] float32: ss = 0; ss += (double)pixel * k tap by tap; stored as float32."""
    src = img.astype(np.float64)
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.float32)
    for i, (lo, cnt) in enumerate(bounds):
        ss = np.zeros(img.shape[1:], np.float64)
        for x in range(cnt):
            ss = ss + src[lo + x] * kk[i, x]
        out[i] = ss.astype(np.float32)
    return out


def resize_clean(img: np.ndarray) -> np.ndarray:
    """[h][w][3] uint8 -> [299][299][3] float32 in 0 .. 255: Pillow's `Image.fromarray(plane, "F").resize((299, 299), Image.BICUBIC)` of every
    plane, bit for bit (horizontal pass first), then the clip to [0, 255]."""
    h, w = img.shape[:2]
    x = img.astype(np.float32)
    if w != SIZE:
        x = _clean_pass(x.transpose(1, 0, 2), *clean_tables(w)).transpose(1, 0, 2)
    if h != SIZE:
        x = _clean_pass(x, *clean_tables(h))
    return np.clip(np.ascontiguousarray(x), np.float32(0), np.float32(255))


def _fma32(a, b, c):
    """fmaf of float32 operands: the product is exact in double, so one rounding to float32 is left (up to a double rounding of the sum)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def legacy_tables(size_in: int, size_out: int = SIZE) -> Tuple[np.ndarray, np.ndarray]:
    """torch's bilinear source indices and weights (align_corners=False, no antialias) in fp32, as its CPU kernels compute them where the
    processor has fused multiply-adds: src = fmaf(scale, i + 0.5, -0.5) with scale = (float)in / out, clamped at 0; idx [out][2] int32 and
    lam [out][2] float32 = (1 - l, l)."""
    f = np.float32
    scale = f(size_in) / f(size_out)
    idx = np.zeros((size_out, 2), np.int32)
    lam = np.zeros((size_out, 2), np.float32)
    for i in range(size_out):
        real = f(float(scale) * float(f(i) + f(0.5)) - 0.5)   # exact in double, rounded once
        if real < 0:
            real = f(0)
        i0 = min(int(np.floor(real)), size_in - 1)
        l1 = min(max(f(real - f(i0)), f(0)), f(1))
        idx[i] = (i0, min(i0 + 1, size_in - 1))
        lam[i] = (f(1) - l1, l1)
    return idx, lam


def resize_legacy(img: np.ndarray) -> np.ndarray:
    """[h][w][3] uint8 -> [299][299][3] float32 in 0 .. 1: torch's F.interpolate(v / 255, (299, 299), mode="bilinear", align_corners=False) in fp32,
    bit for bit: r_k = fmaf(p_k0, wx0, p_k1 * wx1) for the two rows, then fmaf(r_0, wy0, r_1 * wy1)."""
    h, w = img.shape[:2]
    x = img.astype(np.float32) / np.float32(255)
    yi, yl = legacy_tables(h)
    xi, xl = legacy_tables(w)
    rows = []
    for r in range(2):
        g = x[yi[:, r]]
        rows.append(_fma32(g[:, xi[:, 0]], xl[:, 0][None, :, None], g[:, xi[:, 1]] * xl[:, 1][None, :, None]))
    return _fma32(rows[0], yl[:, 0][:, None, None], rows[1] * yl[:, 1][:, None, None])


def network_input(img: np.ndarray, mode: str = "clean") -> np.ndarray:
    """[h][w][3] uint8 -> the network's [299][299][3] float32 input."""
    if mode == "clean":
        return (resize_clean(img) - np.float32(128)) / np.float32(128)
    if mode == "legacy":
        return np.float32(2) * resize_legacy(img) - np.float32(1)
    raise ValueError(f"fid resize mode {mode!r}: clean or legacy")


# ---------------------------------------------------------------- the network
class InceptionFID:
    """The network on the CPU (or `device`) in `dtype`. weights: what load_weights() returns (or takes). features(x) takes [n][299][299][3] inputs and
    returns ([n][2048], the list of the thirteen BLOCKS' per-channel spatial means). The keyword variants exist for the tests that show each known
    way to get FID wrong lands outside the gate; the definition is the defaults."""

    def __init__(self, weights, dtype="fp32", device="cpu", eps=EPS, count_include_pad=False, last_pool_max=True, swap_branches=False):
        import torch
        self.torch = torch
        self.dtype = {"fp32": torch.float32, "fp64": torch.float64}[dtype] if isinstance(dtype, str) else dtype
        w = weights if isinstance(weights, dict) and all(k in weights for k in tensor_names()) else load_weights(weights)
        self.p = {k: torch.as_tensor(v).to(device=device, dtype=self.dtype) for k, v in w.items()}
        self.eps, self.cip, self.last_max, self.swap = eps, count_include_pad, last_pool_max, swap_branches
        self.spec = {name: (stride, (ph, pw)) for name, _, _, _, _, stride, ph, pw in CONVS}

    def conv(self, name, x):
        F = self.torch.nn.functional
        stride, pad = self.spec[name]
        p = self.p
        x = F.conv2d(x, p[f"fid.{name}.w"], None, stride, pad)
        x = F.batch_norm(x, p[f"fid.{name}.bn_mean"], p[f"fid.{name}.bn_var"], p[f"fid.{name}.bn_w"], p[f"fid.{name}.bn_b"], False, 0.0, self.eps)
        return F.relu(x)

    def _avg(self, x):
        return self.torch.nn.functional.avg_pool2d(x, 3, 1, 1, count_include_pad=self.cip)

    def block_a(self, n, x):
        c = self.conv
        out = [c(f"{n}.branch1x1", x), c(f"{n}.branch5x5_2", c(f"{n}.branch5x5_1", x)),
               c(f"{n}.branch3x3dbl_3", c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))), c(f"{n}.branch_pool", self._avg(x))]
        if self.swap and n == "Mixed_5c":
            out[0], out[1] = out[1], out[0]
        return self.torch.cat(out, 1)

    def block_b(self, n, x):
        c = self.conv
        return self.torch.cat([c(f"{n}.branch3x3", x), c(f"{n}.branch3x3dbl_3", c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))),
                               self.torch.nn.functional.max_pool2d(x, 3, 2)], 1)

    def block_c(self, n, x):
        c = self.conv
        d = x
        for k in range(1, 6):
            d = c(f"{n}.branch7x7dbl_{k}", d)
        return self.torch.cat([c(f"{n}.branch1x1", x), c(f"{n}.branch7x7_3", c(f"{n}.branch7x7_2", c(f"{n}.branch7x7_1", x))), d,
                               c(f"{n}.branch_pool", self._avg(x))], 1)

    def block_d(self, n, x):
        c = self.conv
        d = x
        for k in range(1, 5):
            d = c(f"{n}.branch7x7x3_{k}", d)
        return self.torch.cat([c(f"{n}.branch3x3_2", c(f"{n}.branch3x3_1", x)), d, self.torch.nn.functional.max_pool2d(x, 3, 2)], 1)

    def block_e(self, n, x, use_max):
        c = self.conv
        b = c(f"{n}.branch3x3_1", x)
        d = c(f"{n}.branch3x3dbl_2", c(f"{n}.branch3x3dbl_1", x))
        pool = self.torch.nn.functional.max_pool2d(x, 3, 1, 1) if use_max else self._avg(x)
        return self.torch.cat([c(f"{n}.branch1x1", x), c(f"{n}.branch3x3_2a", b), c(f"{n}.branch3x3_2b", b), c(f"{n}.branch3x3dbl_3a", d),
                               c(f"{n}.branch3x3dbl_3b", d), c(f"{n}.branch_pool", pool)], 1)

    def features(self, x):
        torch = self.torch
        F = torch.nn.functional
        means = []

        def keep(t):
            means.append(t.to(torch.float64).mean((2, 3)))
            return t
        with torch.no_grad():
            x = torch.as_tensor(x).to(device=next(iter(self.p.values())).device, dtype=self.dtype).permute(0, 3, 1, 2).contiguous()
            x = keep(self.conv("Conv2d_2b_3x3", self.conv("Conv2d_2a_3x3", self.conv("Conv2d_1a_3x3", x))))
            x = keep(self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", F.max_pool2d(x, 3, 2))))
            x = F.max_pool2d(x, 3, 2)
            for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
                x = keep(self.block_a(n, x))
            x = keep(self.block_b("Mixed_6a", x))
            for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = keep(self.block_c(n, x))
            x = keep(self.block_d("Mixed_7a", x))
            x = keep(self.block_e("Mixed_7b", x, False))
            x = keep(self.block_e("Mixed_7c", x, self.last_max))
        return means[-1].cpu().numpy(), [m.cpu().numpy() for m in means]

    def features_of_images(self, images: Sequence[np.ndarray], mode="clean", batch=8) -> np.ndarray:
        out = []
        for i in range(0, len(images), batch):
            x = np.stack([network_input(im, mode) for im in images[i:i + batch]])
            out.append(self.features(x)[0])
        return np.concatenate(out) if out else np.zeros((0, DIM))


# ---------------------------------------------------------------- the set level
class FidError(ValueError):
    pass


def statistics(features: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """mu [D] and sigma [D][D] = np.cov(features, rowvar=False) (ddof 1) of [N][D] features, fp64."""
    f = np.asarray(features, np.float64)
    if f.ndim != 2 or f.shape[0] < 2:
        raise FidError(f"FID needs at least 2 files on either side, got {0 if f.ndim != 2 else f.shape[0]}")
    return f.mean(0), np.atleast_2d(np.cov(f, rowvar=False))


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape or s1.shape != (mu1.size, mu1.size):
        raise FidError(f"FID: statistics of different sizes ({mu1.shape}, {s1.shape} against {mu2.shape}, {s2.shape})")
    lam, q = np.linalg.eigh((s1 + s1.T) / 2)
    lam = np.where(lam > _rank_floor(lam), lam, 0.0)   # the null space of a singular covariance is rounding noise: its roots would not be
    root = (q * np.sqrt(lam)) @ q.T
    m = root @ ((s2 + s2.T) / 2) @ root
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    ev = np.where(ev > _rank_floor(ev), ev, 0.0)
    d = mu1 - mu2
    return max(float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(ev).sum()), 0.0)   # d^2 >= 0; rounding may leave -1e-13 for equal sets


def _rank_floor(lam: np.ndarray) -> float:
    """Eigenvalues of a positive semi-definite matrix at or below this are zero to working precision (numpy.linalg.matrix_rank's rule)."""
    return float(np.abs(lam).max(initial=0.0)) * lam.size * np.finfo(np.float64).eps


def load_stats(path) -> Tuple[np.ndarray, np.ndarray]:
    """pytorch-fid's statistics file: `mu` [D] and `sigma` [D][D]."""
    with np.load(path) as z:
        if "mu" not in z.files or "sigma" not in z.files:
            raise FidError(f"{path}: not a statistics file (mu and sigma are needed, it has {sorted(z.files)})")
        mu, sigma = np.asarray(z["mu"], np.float64), np.asarray(z["sigma"], np.float64)
    if mu.ndim != 1 or sigma.shape != (mu.size, mu.size):
        raise FidError(f"{path}: mu {mu.shape} and sigma {sigma.shape} do not belong together")
    return mu, sigma


class FeatureSet:
    """Names + [N][D] float64 features of one side of a run; saved as .npz (`names`, `features`)."""

    def __init__(self, dim: int = DIM):
        self.names: List[str] = []
        self.rows: List[np.ndarray] = []
        self.dim = dim

    def add(self, name: str, feature) -> None:
        f = np.asarray(feature, np.float64).reshape(-1)
        if f.size != self.dim:
            raise FidError(f"{name}: a feature of {f.size} values, the set holds {self.dim}")
        self.names.append(str(name))
        self.rows.append(f.copy())

    def __len__(self):
        return len(self.names)

    @property
    def features(self) -> np.ndarray:
        return np.stack(self.rows) if self.rows else np.zeros((0, self.dim))

    def save(self, path, **extra) -> None:
        with open(path, "wb") as f:
            np.savez(f, names=np.array(self.names, dtype=np.str_), features=self.features, **extra)

    @classmethod
    def load(cls, path, key="features", names_key="names") -> "FeatureSet":
        with np.load(path) as z:
            if key not in z.files:
                raise FidError(f"{path}: no `{key}` in it ({sorted(z.files)})")
            feats = np.asarray(z[key], np.float64)
            names = [str(s) for s in z[names_key]] if names_key in z.files else [str(i) for i in range(feats.shape[0])]
        out = cls(feats.shape[1] if feats.ndim == 2 else DIM)
        for n, f in zip(names, feats):
            out.add(n, f)
        return out


def merge(sets: Sequence[FeatureSet]) -> FeatureSet:
    """One set out of several (the ranks' files), ordered by name so that the result does not depend on how the files were split."""
    sets = list(sets)
    out = FeatureSet(sets[0].dim if sets else DIM)
    rows = sorted(((n, i, j) for i, s in enumerate(sets) for j, n in enumerate(s.names)), key=lambda t: t[0])
    for n, i, j in rows:
        out.add(n, sets[i].rows[j])
    return out


def rank_deficient_note(n: int, dim: int = DIM) -> Optional[str]:
    if n < dim:
        return f"note on fid: {n} files against {dim} feature dimensions: the covariance is rank-deficient and the value is only comparable at equal N"
    return None


def fid_of(features_a: np.ndarray, features_b: Optional[np.ndarray] = None, stats=None) -> float:
    mu1, s1 = statistics(features_a)
    mu2, s2 = stats if stats is not None else statistics(features_b)
    return frechet_distance(mu1, s1, mu2, s2)


# ---------------------------------------------------------------- command line
IMAGE_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")


def _folder(path) -> List[str]:
    """The image files of a folder and of its sub-folders (a run mirrors its input tree), sorted."""
    return sorted(os.path.join(root, f) for root, _, names in os.walk(path) for f in names if f.lower().endswith(IMAGE_EXT))


def _load_rgb(path) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _gpu_features(model, files, mode) -> np.ndarray:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from instarevive_amd import fid as G
    import torch
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    G.configure(ctx, model)
    return np.stack([G.fid_arrays(ctx, _load_rgb(f), mode)[0] for f in files]) if files else np.zeros((0, DIM))


def folder_features(model, files, mode, dtype, backend) -> np.ndarray:
    if backend == "gpu":
        return _gpu_features(model, files, mode)
    net = InceptionFID(model, dtype)
    return net.features_of_images([_load_rgb(f) for f in files], mode, 4)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("folders", nargs="*", help="RESULTS [REFERENCE]")
    ap.add_argument("--model", help="pytorch-fid's pt_inception weights (.pth state dict) or an .npz in ir_fid_configure's names")
    ap.add_argument("--stats", help="reference statistics (.npz with mu and sigma) in place of the REFERENCE folder")
    ap.add_argument("--save_stats", help="write the statistics of RESULTS (mu, sigma) to this .npz")
    ap.add_argument("--features", nargs="+", help="feature files of a run (the ranks' fid_features*.npz) in place of RESULTS")
    ap.add_argument("--resize", choices=("clean", "legacy"), default="clean")
    ap.add_argument("--dtype", choices=("fp32", "fp64"), default="fp32")
    ap.add_argument("--backend", choices=("cpu", "gpu"), default="cpu")
    a = ap.parse_args(argv)
    try:
        ref = None
        if a.features:
            sets = [FeatureSet.load(f) for f in a.features]
            fa = merge(sets).features
            if not a.stats and not a.folders:
                refs = []
                for f in a.features:
                    with np.load(f) as z:
                        if "gt_features" in z.files:
                            refs.append(FeatureSet.load(f, "gt_features", "gt_names"))
                ref = merge(refs).features if refs else None
        else:
            if not a.folders or not a.model:
                ap.error("RESULTS and --model are needed (or --features)")
            fa = folder_features(a.model, _folder(a.folders[0]), a.resize, a.dtype, a.backend)
        if a.save_stats:
            mu, sigma = statistics(fa)
            with open(a.save_stats, "wb") as f:
                np.savez(f, mu=mu, sigma=sigma)
            print(f"statistics of {fa.shape[0]} files -> {a.save_stats}")
        if a.stats:
            stats = load_stats(a.stats)
        else:
            if ref is None and not a.features and len(a.folders) == 2:
                ref = folder_features(a.model, _folder(a.folders[1]), a.resize, a.dtype, a.backend)
            if ref is None:
                if a.save_stats:
                    return 0
                ap.error("a REFERENCE folder or --stats is needed")
            stats = statistics(ref)
        note = rank_deficient_note(fa.shape[0])
        if note:
            print(note)
        print(f"fid: {frechet_distance(*statistics(fa), *stats):.5f}")
    except (FidError, KeyError, OSError) as e:
        print(f"evaluate_fid: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
