#!/usr/bin/env python3
"""Paired metrics of an output folder against a ground-truth folder: the PSNR-Y / SSIM-Y / LPIPS half of the reference's evaluate_img.py
(/root/reference/evaluate_img.py:30-33 creates them, :40-57 averages them over the sorted file lists).

    python tools/evaluate_pairs.py -i results/ -r gt/ [--ntest N] [--lpips_alexnet alexnet-owt-7be5be79.pth --lpips_lin alex.pth]
                                   [--dists_model DISTS_weights.pt --dists_vgg vgg16-397923af.pth]

The reference takes all three from pyiqa (`create_metric('psnr' | 'ssim', test_y_channel=True, color_space='ycbcr')`, `create_metric('lpips')`);
its training code wraps the `lpips` package itself (utils/metrics.py:41-66, `LPIPS(net="alex")`). Neither package is in this image or in the
reference tree, so their definitions are RESTATED here from the published implementations - parity unpinned until a box with pyiqa / lpips
runs tools/repin_with_diffusers.py-style checks:
  * Y = (16 + 65.481 R + 128.553 G + 24.966 B) / 255 (BT.601 studio swing; R, G, B in [0, 1]);
  * PSNR (pyiqa `psnr`, data_range 1 - its default, which evaluate_img.py does not override): Y on the UNIT scale, no rounding,
    10 log10(1 / (mean((Yx - Yy)^2) + 1e-8));
  * SSIM (pyiqa `ssim` works on the 0..255 scale whatever the input range): Y x 255 ROUNDED to integers, 11 x 11 Gaussian window (sigma 1.5),
    'valid' filtering, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, the contrast-structure term clamped at 0, mean over the map; no down-sampling;
  * LPIPS v0.1, net 'alex' (the default of both packages): inputs [0, 1] -> [-1, 1] (normalize=True), the scaling layer
    (x - (-.030, -.088, -.188)) / (.458, .448, .450), the five ReLU outputs of torchvision's AlexNet `features` (conv 11/4 pad 2 -> pool 3/2 ->
    conv 5 pad 2 -> pool 3/2 -> conv 3 -> conv 3 -> conv 3), each unit-normalised over channels (x / (|x|_2 + 1e-10)), squared differences
    weighted by a non-negative 1 x 1 "lin" layer per stage, averaged over space, summed over the five stages.
    The pretrained weights (torchvision's alexnet-owt-7be5be79.pth, 233 MB, and lpips/weights/v0.1/alex.pth, 6 KB) do not exist offline:
    LPIPS is computed only when the user passes them (--lpips_alexnet / --lpips_lin, or one full `lpips.LPIPS().state_dict()` file through
    --lpips_lin alone); the arithmetic is tested against an independent torch.nn construction on random weights (tests/test_host_cpu.py).
  * DISTS (not in evaluate_img.py; the column papers print next to LPIPS, pyiqa's `dists` at its defaults): `class DISTS` below states the whole
    definition; computed only when the user passes the weights (--dists_model [--dists_vgg]).
Of the no-reference metrics of the same script, MANIQA, MUSIQ and CLIPIQA are pretrained networks: each has its own tool,
tools/evaluate_clipiqa.py, tools/evaluate_musiq.py and tools/evaluate_maniqa.py (its 20 crops lie on pyiqa's uniform grid, or are drawn from a
seed and the file's name), which take the user's weights. NIQE
is classical image statistics plus a few KB of pristine parameters and has its own tool, tools/evaluate_niqe.py.
Files are paired by sorted order exactly as the reference does (glob "*.[jpJP][pnPN]*[gG]")."""
import argparse
import sys
from pathlib import Path

import numpy as np


def to_y(img_rgb01: np.ndarray, data_range: float = 255.0) -> np.ndarray:
    """HWC float RGB in [0, 1] -> Y of YCbCr (BT.601 studio swing) on the 0..data_range scale (fp64); rounded to integers on the 255
    scale only (pyiqa.utils.color_util.to_y_channel rounds when out_data_range >= 255 and not otherwise)."""
    x = np.asarray(img_rgb01, np.float64)
    y = (16.0 + 65.481 * x[..., 0] + 128.553 * x[..., 1] + 24.966 * x[..., 2]) / 255.0 * data_range
    return np.round(y) if data_range >= 255 else y


def psnr_y(a_rgb01, b_rgb01) -> float:
    """pyiqa `psnr(test_y_channel=True, color_space='ycbcr')` at its default data_range 1: unit-scale Y, no rounding, eps on the unit MSE."""
    d = to_y(a_rgb01, 1.0) - to_y(b_rgb01, 1.0)
    return float(10.0 * np.log10(1.0 / (np.mean(d * d) + 1e-8)))


def _gauss_window(size=11, sigma=1.5):
    c = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-(c * c) / (2 * sigma * sigma))
    g /= g.sum()
    return g


def _filter_valid(x, g):
    """Separable 'valid' correlation with the 1-D window g along both axes."""
    k = len(g)
    h, w = x.shape
    tmp = np.zeros((h - k + 1, w), np.float64)
    for i in range(k):
        tmp += g[i] * x[i:i + h - k + 1]
    out = np.zeros((h - k + 1, w - k + 1), np.float64)
    for i in range(k):
        out += g[i] * tmp[:, i:i + w - k + 1]
    return out


def ssim_y(a_rgb01, b_rgb01) -> float:
    x, y = to_y(a_rgb01), to_y(b_rgb01)
    if x.shape != y.shape:
        raise ValueError(f"image shapes differ: {x.shape} vs {y.shape}")
    if min(x.shape) < 11:
        raise ValueError("SSIM needs images of at least 11 x 11 pixels")
    g = _gauss_window()
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    mu1, mu2 = _filter_valid(x, g), _filter_valid(y, g)
    s11 = _filter_valid(x * x, g) - mu1 * mu1
    s22 = _filter_valid(y * y, g) - mu2 * mu2
    s12 = _filter_valid(x * y, g) - mu1 * mu2
    cs = np.maximum((2 * s12 + c2) / (s11 + s22 + c2), 0.0)
    return float(np.mean((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * cs))


# ---------------------------------------------------------------------------------------------------------------- LPIPS (v0.1, alex)
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))  # features idx, cin, cout, k, stride, pad
ALEX_POOL_BEFORE = (False, True, True, False, False)   # MaxPool2d(3, 2) in front of conv2 and conv3 (torchvision features.2 / features.5)
# full-model key of each backbone conv in lpips.LPIPS().state_dict(): the slices keep torchvision's indices
LPIPS_SLICE_KEY = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")


class LPIPS:
    """lpips.LPIPS(net='alex', version='0.1') in eval mode, restated (utils/metrics.py:41-66 wraps it; evaluate_img.py:32 takes pyiqa's copy of
    the same network). Weights come from the user's files: `alexnet` = torchvision's AlexNet state dict (`features.N.weight|bias`) and `lin` = the
    lpips linear heads (`lin{k}.model.1.weight`, [1, C, 1, 1]); or `lin` alone holding a full lpips state dict (`net.slice*.N.*` + `lin*`)."""

    def __init__(self, alexnet=None, lin=None, device="cpu"):
        import torch
        sd = {}
        for src in (alexnet, lin):
            if src is None:
                continue
            part = torch.load(src, map_location="cpu") if isinstance(src, (str, Path)) else src
            sd.update(part.get("state_dict", part) if isinstance(part, dict) else part)
        self.convs, self.lins = [], []
        for k, (idx, cin, cout, ks, _, _) in enumerate(ALEX_CONVS):
            for base in (f"features.{idx}", LPIPS_SLICE_KEY[k]):
                if base + ".weight" in sd:
                    w, b = sd[base + ".weight"], sd[base + ".bias"]
                    break
            else:
                raise KeyError(f"AlexNet conv {k + 1}: neither features.{idx}.weight nor {LPIPS_SLICE_KEY[k]}.weight in the given files")
            lw = sd.get(f"lin{k}.model.1.weight")
            if lw is None:
                raise KeyError(f"lin{k}.model.1.weight missing: pass the lpips linear heads (lpips/weights/v0.1/alex.pth)")
            if tuple(w.shape) != (cout, cin, ks, ks) or tuple(lw.shape) != (1, cout, 1, 1):
                raise ValueError(f"stage {k}: conv {tuple(w.shape)} / lin {tuple(lw.shape)} are not AlexNet's")
            self.convs.append((w.to(device, torch.float32), b.to(device, torch.float32)))
            self.lins.append(lw.to(device, torch.float32))
        self.shift = torch.tensor([-.030, -.088, -.188], device=device).view(1, 3, 1, 1)
        self.scale = torch.tensor([.458, .448, .450], device=device).view(1, 3, 1, 1)
        self.device = device

    def features(self, x):
        import torch.nn.functional as F
        outs = []
        for (w, b), (_, _, _, _, stride, pad), pool in zip(self.convs, ALEX_CONVS, ALEX_POOL_BEFORE):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
            outs.append(x)
        return outs

    def __call__(self, img1, img2, normalize=True):
        """img1, img2: NCHW RGB tensors, [0, 1] with normalize=True (pyiqa's and evaluate_img.py's use), [-1, 1] otherwise -> [N] distances."""
        import torch
        with torch.no_grad():
            a, b = (t.to(self.device, torch.float32) for t in (img1, img2))
            if normalize:
                a, b = 2 * a - 1, 2 * b - 1
            fa, fb = self.features((a - self.shift) / self.scale), self.features((b - self.shift) / self.scale)
            total = 0
            for xa, xb, lw in zip(fa, fb, self.lins):
                na = xa / (xa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                nb = xb / (xb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                total = total + ((na - nb) ** 2 * lw).sum(1, keepdim=True).mean((2, 3), keepdim=True)
            return total.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- DISTS
VGG_STAGES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))   # torchvision VGG-16 `features` indices of the convs of each stage
VGG_WIDTHS = (64, 128, 256, 512, 512)
DISTS_CHNS = (3,) + VGG_WIDTHS                                             # the six compared maps: the raw image, then each stage's output
DISTS_MEAN = (0.485, 0.456, 0.406)
DISTS_STD = (0.229, 0.224, 0.225)


class DISTS:
    """DISTS (Ding, Ma, Wang, Simoncelli: "Image Quality Assessment: Unifying Structure and Texture Similarity") as the published model and
    pyiqa's `dists` compute it at their defaults - no resize, the image's own size, eval mode - restated; the model of ir_dists.
      input x = v / 255 in [0, 1]; network input (x - mean) / std, every step rounded to float32 whatever `dtype` is;
      five stages of torchvision VGG-16 `features` (3x3 convs, stride 1, zero padding 1, bias, ReLU): 3 -> 64 -> 64 | 128, 128 | 256 x 3 | 512 x 3 |
      512 x 3, with an L2 pool in front of stages 2 .. 5: per channel sqrt(conv2d(x * x, g, stride 2, zero padding 1) + 1e-12) with
      g = outer(a, a) / sum, a = hanning(5)[1:-1] = (0.5, 1, 0.5), i.e. (1, 2, 1) x (1, 2, 1) / 16, the nine taps added row by row from the
      top-left; the output is ceil(H / 2) x ceil(W / 2);
      six maps are compared - the raw x (3 channels, not the normalised input) and the ReLU output that ends each stage, 1475 channels - per
      channel over the map's own pixels: mx, my the means, vx = mean((fx - mx)^2), vy (biased), cxy = mean(fx fy) - mx my,
      S1 = (2 mx my + 1e-6) / (mx^2 + my^2 + 1e-6), S2 = (2 cxy + 1e-6) / (vx + vy + 1e-6);
      score = 1 - sum_c (alpha_c S1_c + beta_c S2_c) / (sum(alpha) + sum(beta)).
    Weights come from the user's files: `weights` = one state dict in the DISTS module's names (`stage1.0.weight` .. `stage5.28.bias`, `alpha`,
    `beta` [1, 1475, 1, 1]; the `mean`, `std` and `*.filter` buffers are ignored), or `alpha` / `beta` alone (DISTS_weights.pt) with `vgg` =
    torchvision's vgg16-397923af.pth (`features.N.*`; the classifier is ignored). dtype: torch.float32 (default) or torch.float64."""

    def __init__(self, weights=None, vgg=None, device="cpu", dtype=None):
        import torch
        sd = {}
        for src in (vgg, weights):
            if src is None:
                continue
            part = torch.load(src, map_location="cpu") if isinstance(src, (str, Path)) else src
            sd.update(part.get("state_dict", part) if isinstance(part, dict) else part)
        self.dtype = dtype or torch.float32
        self.device = device
        self.stages, cin = [], 3
        for k, (idxs, cout) in enumerate(zip(VGG_STAGES, VGG_WIDTHS)):
            convs = []
            for idx in idxs:
                for base in (f"stage{k + 1}.{idx}", f"features.{idx}"):
                    if base + ".weight" in sd:
                        w, b = sd[base + ".weight"], sd[base + ".bias"]
                        break
                else:
                    raise KeyError(f"VGG-16 conv features.{idx}: neither stage{k + 1}.{idx}.weight nor features.{idx}.weight in the given files")
                if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                    raise ValueError(f"features.{idx}: conv {tuple(w.shape)} / bias {tuple(b.shape)} are not VGG-16's")
                convs.append((w.to(device, self.dtype), b.to(device, self.dtype)))
                cin = cout
            self.stages.append(convs)
        for name in ("alpha", "beta"):
            if name not in sd:
                raise KeyError(f"{name} missing: pass the DISTS weights (DISTS_weights.pt)")
            if sd[name].numel() != sum(DISTS_CHNS):
                raise ValueError(f"{name} has {sd[name].numel()} entries, DISTS has {sum(DISTS_CHNS)}")
            setattr(self, name, sd[name].reshape(-1).to(device, self.dtype))
        self.mean = torch.tensor(DISTS_MEAN, device=device).view(1, 3, 1, 1)
        self.std = torch.tensor(DISTS_STD, device=device).view(1, 3, 1, 1)
        a = torch.tensor([0.5, 1.0, 0.5], dtype=self.dtype, device=device)   # hanning(5)[1:-1]
        self.window = (a[:, None] * a[None, :]) / (a[:, None] * a[None, :]).sum()

    def l2pool(self, x):
        import torch.nn.functional as F
        c = x.shape[1]
        return (F.conv2d(x * x, self.window.expand(c, 1, 3, 3).contiguous(), stride=2, padding=1, groups=c) + 1e-12).sqrt()

    def maps(self, x01):
        """x01: NCHW float32 in [0, 1] -> the six compared maps in self.dtype."""
        import torch
        import torch.nn.functional as F
        assert x01.dtype == torch.float32
        outs = [x01.to(self.dtype)]
        h = ((x01 - self.mean) / self.std).to(self.dtype)   # float32 roundings, then the model's precision
        for k, convs in enumerate(self.stages):
            if k:
                h = self.l2pool(h)
            for w, b in convs:
                h = F.relu(F.conv2d(h, w, b, padding=1))
            outs.append(h)
        return outs

    def moments(self, fx, fy):
        """[N][C][5]: mx, my, vx, vy, cxy of one map of either image."""
        import torch
        mx, my = fx.mean((2, 3), keepdim=True), fy.mean((2, 3), keepdim=True)
        vx, vy = ((fx - mx) ** 2).mean((2, 3)), ((fy - my) ** 2).mean((2, 3))
        cxy = (fx * fy).mean((2, 3)) - mx[..., 0, 0] * my[..., 0, 0]
        return torch.stack((mx[..., 0, 0], my[..., 0, 0], vx, vy, cxy), -1)

    def all_moments(self, img1, img2):
        """img1, img2: NCHW RGB tensors in [0, 1] -> [N][1475][5], channels in map order."""
        import torch
        with torch.no_grad():
            a, b = (t.to(self.device, torch.float32) for t in (img1, img2))
            return torch.cat([self.moments(fx, fy) for fx, fy in zip(self.maps(a), self.maps(b))], 1)

    def score(self, m):
        """[N][1475][5] moments -> [N] scores."""
        mx, my, vx, vy, cxy = m.unbind(-1)
        s1 = (2 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6)
        s2 = (2 * cxy + 1e-6) / (vx + vy + 1e-6)
        one = s1.new_ones(s1.shape)   # the weights are summed as the weighted terms are: S1 = S2 = 1 then gives exactly 0
        return 1 - ((self.alpha * s1).sum(1) + (self.beta * s2).sum(1)) / ((self.alpha * one).sum(1) + (self.beta * one).sum(1))

    def __call__(self, img1, img2):
        return self.score(self.all_moments(img1, img2))


def list_images(folder):
    return sorted(Path(folder).glob("*.[jpJP][pnPN]*[gG]"))


def _gpu_scorer():
    """--backend gpu: PSNR-Y / SSIM-Y of a pair from the device kernel (ir_metrics_y) that follows the definitions above."""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from instarevive_amd.metrics import score_arrays
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    return lambda a8, b8: score_arrays(ctx, a8, b8)


def _gpu_lpips(alexnet, lin):
    """--backend gpu with LPIPS weights: the distance of a pair from the device kernel (ir_lpips, exact fp32) in place of the torch model."""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from instarevive_amd import lpips as device_lpips
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    device_lpips.configure(ctx, lin, alexnet)
    return lambda a8, b8: device_lpips.lpips_arrays(ctx, a8, b8)


def _gpu_dists(model, vgg):
    """--backend gpu with DISTS weights: the score of a pair from the device kernel (ir_dists, exact fp32 convolutions, fp64 statistics)."""
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from instarevive_amd import dists as device_dists
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    device_dists.configure(ctx, model, vgg)
    return lambda a8, b8: device_dists.dists_arrays(ctx, a8, b8)


def evaluate(in_path, ref_path, ntest=None, log=print, lpips=None, backend="host", lpips_u8=None, dists=None, dists_u8=None):
    """lpips: the torch model (img1, img2 in [0, 1]); lpips_u8: a scorer of two HWC uint8 arrays in its place (the device's). dists / dists_u8:
    the same two forms of DISTS; its line comes last."""
    from PIL import Image
    ins, refs = list_images(in_path), list_images(ref_path)
    if ntest is not None:
        ins, refs = ins[:ntest], refs[:ntest]
    if not ins or len(ins) != len(refs):
        raise SystemExit(f"{len(ins)} images in {in_path}, {len(refs)} in {ref_path}: the folders must pair up (sorted order, as evaluate_img.py)")
    log(f"Find {len(ins)} images in {in_path}")
    tot = {"psnr": 0.0, "ssim": 0.0}
    if lpips_u8 is not None:
        tot["lpips"] = 0.0
    elif lpips is not None:
        import torch
        tot["lpips"] = 0.0
    if dists is not None or dists_u8 is not None:
        import torch
        tot["dists"] = 0.0
    score = _gpu_scorer() if backend == "gpu" else None
    for fi, fr in zip(ins, refs):
        a8, b8 = np.asarray(Image.open(fi).convert("RGB")), np.asarray(Image.open(fr).convert("RGB"))
        a = np.asarray(a8, np.float32) / 255.0
        b = np.asarray(b8, np.float32) / 255.0
        if a.shape != b.shape:
            raise SystemExit(f"{fi.name} {a.shape} and {fr.name} {b.shape} differ in size")
        if score is not None:
            p, s = score(a8, b8)
            tot["psnr"] += p
            tot["ssim"] += s
        else:
            tot["psnr"] += psnr_y(a, b)
            tot["ssim"] += ssim_y(a, b)
        if lpips_u8 is not None:
            tot["lpips"] += float(lpips_u8(a8, b8))
        elif lpips is not None:
            tot["lpips"] += float(lpips(torch.from_numpy(a).permute(2, 0, 1)[None], torch.from_numpy(b).permute(2, 0, 1)[None], normalize=True)[0])
        if dists_u8 is not None:
            tot["dists"] += float(dists_u8(a8, b8))
        elif dists is not None:
            tot["dists"] += float(dists(torch.from_numpy(a).permute(2, 0, 1)[None], torch.from_numpy(b).permute(2, 0, 1)[None])[0])
    res = {k: v / len(ins) for k, v in tot.items()}
    for k, v in res.items():
        log(f"{k}: {v:.5f}")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-i", "--in_path", type=str, required=True)
    ap.add_argument("-r", "--ref_path", type=str, required=True)
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--lpips_alexnet", type=str, default=None, help="torchvision AlexNet state dict (alexnet-owt-7be5be79.pth)")
    ap.add_argument("--lpips_lin", type=str, default=None, help="lpips v0.1 linear heads (lpips/weights/v0.1/alex.pth), or a full lpips.LPIPS() state dict")
    ap.add_argument("--dists_model", type=str, default=None, help="score DISTS as well (class DISTS; the line `dists:` comes last): one state dict in the DISTS "
                    "module's names, or alpha / beta alone (DISTS_weights.pt) with --dists_vgg; with --backend gpu also an .npz in ir_dists_configure's names")
    ap.add_argument("--dists_vgg", type=str, default=None, help="with --dists_model holding alpha / beta alone: torchvision's VGG-16 state dict (vgg16-397923af.pth)")
    ap.add_argument("--device", type=str, default="cpu")
    ap.add_argument("--backend", type=str, default="host", choices=["host", "gpu"], help="who computes PSNR-Y / SSIM-Y: host (default) = the numpy fp64 "
                    "definitions of this file; gpu = ir_metrics_y on the MI355X (the same definitions, fp64 statistics; the printed lines are the same) and, with --lpips_lin, "
                    "LPIPS from ir_lpips (exact fp32 convolutions, fp64 sums: within 1e-6 relative of the torch model, so a last printed digit may differ) and, with "
                    "--dists_model, DISTS from ir_dists (within 2e-6 absolute of the torch model)")
    a = ap.parse_args()
    if a.dists_vgg and not a.dists_model:
        raise SystemExit("--dists_vgg needs --dists_model (DISTS' alpha / beta)")
    more = {}
    if a.dists_model and a.backend == "gpu":
        more["dists_u8"] = _gpu_dists(a.dists_model, a.dists_vgg)
    elif a.dists_model:
        more["dists"] = DISTS(a.dists_model, a.dists_vgg, a.device)
    if a.lpips_lin and a.backend == "gpu":
        evaluate(a.in_path, a.ref_path, a.ntest, backend=a.backend, lpips_u8=_gpu_lpips(a.lpips_alexnet, a.lpips_lin), **more)
        return
    net = LPIPS(a.lpips_alexnet, a.lpips_lin, a.device) if a.lpips_lin else None
    if net is None:
        print("lpips: skipped (no weights given: --lpips_lin [--lpips_alexnet])")
    evaluate(a.in_path, a.ref_path, a.ntest, lpips=net, backend=a.backend, **more)


if __name__ == "__main__":
    sys.exit(main())
