#!/usr/bin/env python3
"""MANIQA of an output folder: the no-reference metric `maniqa` of the reference's evaluate_img.py (`create_metric('maniqa')`).

    python tools/evaluate_maniqa.py -i results/ --maniqa_model maniqa_koniq.npz [--maniqa_crops uniform|random] [--maniqa_seed N] [--backend gpu]

The reference takes it from pyiqa, which is not in this image, and neither timm nor the pretrained checkpoint exists offline: the user passes the
weights. So the definition is RESTATED here as a plain torch model from the published implementation (pyiqa's `maniqa`, i.e. the koniq checkpoint:
scale 0.8, 20 crops, taps 6..9) - parity with pyiqa itself is unpinned until a box that has it runs tools/repin_with_diffusers.py (item 12).
The recollections of pyiqa stand in one named place each: PYIQA_KEYS (the checkpoint's key names), uniform_origins() (the crop grid) and
DEFAULTS (scale, crops, taps). This file is the model ir_maniqa (csrc/maniqa.hip) is tested against; it runs on the CPU in float32 or float64.
The metric is exact fp32 - evaluate_img.py's autocast scoring is not reproduced.

  1. input: RGB bytes v; x = (v / 255 - 0.5) / 0.5 in float32, each step rounded in that order (a 256-entry table for all three channels).
  2. crops: `crops` windows of crop x crop pixels at the origins (y, x) of crop_origins(): mode "uniform" is pyiqa's uniform_crop - step =
     (side - crop) // floor(sqrt(crops)) per axis, positions i * step for i < ceil(sqrt(crops)), y outer, x inner, the first `crops` of them;
     mode "random" draws them from numpy's default_rng([seed, crc32(name)]). An image with min(h, w) <= crop is refused (ManiqaError): pyiqa
     enlarges it bilinearly first, which is not offered.
  3. trunk, per crop: timm's vit_base_patch8_224 - a patch x patch stride-patch conv (weights flattened (c, ky, kx)) to embed, the class token in
     front, + pos_embed [1 + N][embed], pre-LN blocks (LayerNorm eps 1e-6, biased q|k|v in one linear, heads of embed / vit_heads, the scores
     (q k^T) * hd^-0.5, exact GELU). Only blocks 0 .. taps[-1] run; the outputs of the blocks `taps`, without the class token, are concatenated
     along the channels to [N][4 embed] and read as X [C = 4 embed][N].
  4. TAB (two in front of each stage) on X [C][N]: q, k, v = Linear(N, N) along N; A = softmax_rows((q k^T) * N^-0.5), a C x C matrix; P = A v
     [C][N]; then P.transpose(0, 1).reshape(C, N) - element [c][n] of P lands at flat offset n * C + c - plus X. The pretrained weights were
     trained with this reinterpretation; it is reproduced as it is.
  5. stage 1: 1 x 1 conv C -> embed, then the Swin stage at embed with MLP width dim_mlp; stage 2 after two more TABs at C = embed: 1 x 1 conv
     embed -> embed / 2, then a Swin stage at embed / 2 with MLP width dim_mlp / 2.
  6. Swin stage on the G x G token grid (G = crop / patch): SWIN_LAYERS = 2 layers of swin_depth blocks, window `window`, block b shifted by
     window / 2 when b is odd; each layer enters as scale * layer(x) + x. Block: x += proj(window_attention(LN1 x)); x += fc2(gelu(fc1(LN2 x))),
     LayerNorm eps 1e-5. Window attention: swin_heads heads, q * hd^-0.5 BEFORE q k^T, + relative_position_bias_table[index] ((2 window - 1)^2
     rows, index = (dy + window - 1) * (2 window - 1) + dx + window - 1 with d = query - key), + (-100) where the two tokens of a shifted window
     carry different region labels (the labels of Swin's img_mask: slices [0, -window), [-window, -shift), [-shift, end) per axis).
  7. heads on the embed / 2 wide tokens: s = relu(fc2(relu(fc1 t))), w = sigmoid(fc2(relu(fc1 t))); the image's score is
     sum(w * s) / (sum(w) + 1e-8) over the patches of ALL its crops together. Dropout is the identity.

The model file: an .npz in the project's own names - the form that always works -
    vit.patch.{weight [embed][3][p][p], bias}, vit.cls_token [embed], vit.pos_embed [1 + N][embed], vit.blocks.L.{ln1,ln2}.{weight,bias},
    vit.blocks.L.attn.qkv.{weight [3 embed][embed], bias}, vit.blocks.L.attn.proj.*, vit.blocks.L.mlp.fc1.* [vit_mlp][embed], vit.blocks.L.mlp.fc2.*;
    tabS.K.{q,k,v}.{weight [N][N], bias} (S = 1, 2; K = 0, 1); convS.{weight [out][in], bias};
    swinS.L.B.{ln1,ln2}.*, swinS.L.B.attn.rpb [(2 window - 1)^2][swin_heads], swinS.L.B.attn.qkv.*, swinS.L.B.attn.proj.*, swinS.L.B.mlp.fc1.*, .mlp.fc2.*;
    score.fc1.*, score.fc2.* [1][embed / 2], weight.fc1.*, weight.fc2.*
    and, optionally, the configuration as cfg.scale, cfg.crops, cfg.taps, cfg.vit_heads, cfg.swin_heads, cfg.patch (else DEFAULTS)
or pyiqa's .pth state dict (plain, or under `params` / `state_dict`; the ViT's tensors under `vit.`; blocks behind the last tap are ignored).
Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import math
import os
import sys
import zlib
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

VIT_LN_EPS, SWIN_LN_EPS, POOL_EPS = 1e-6, 1e-5, 1e-8
SWIN_LAYERS, TABS = 2, 2
MASK = -100.0
# RECALLED FROM PYIQA (DEFAULT_CONFIGS['maniqa'] and MANIQA.__init__), unpinned
DEFAULTS = dict(patch=8, vit_heads=12, swin_heads=4, taps=(6, 7, 8, 9), scale=0.8, crops=20)
DEFAULT_SEED = 231
# what a wrong implementation might do instead, one per step; the tests show that the gate tells each apart
VARIANTS = ("tab_transposed_back", "tab_scale_c", "tab_softmax_axis", "taps_shifted", "taps_keep_cls", "no_shift_mask", "rpb_index_transposed", "vit_ln_eps_1e5",
            "gelu_tanh", "no_scale", "per_crop_mean", "origins_swapped")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ManiqaError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- recollections of pyiqa (unpinned)
def _pyiqa_keys(cfg) -> dict:
    """RECALLED FROM PYIQA (maniqa_arch.MANIQA with timm's VisionTransformer inside), unpinned: {this project's name: the checkpoint's key}."""
    k = {"vit.patch.weight": "vit.patch_embed.proj.weight", "vit.patch.bias": "vit.patch_embed.proj.bias", "vit.cls_token": "vit.cls_token", "vit.pos_embed": "vit.pos_embed"}

    def block(a, b, rpb):
        for v in ("weight", "bias"):
            k[f"{a}ln1.{v}"] = f"{b}norm1.{v}"
            k[f"{a}ln2.{v}"] = f"{b}norm2.{v}"
            for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
                k[f"{a}{n}.{v}"] = f"{b}{n}.{v}"
        if rpb:
            k[f"{a}attn.rpb"] = f"{b}attn.relative_position_bias_table"

    for i in range(cfg["vit_layers"]):
        block(f"vit.blocks.{i}.", f"vit.blocks.{i}.", False)
    for s in (1, 2):
        for t in range(TABS):
            for n in "qkv":
                for v in ("weight", "bias"):
                    k[f"tab{s}.{t}.{n}.{v}"] = f"tablock{s}.{t}.c_{n}.{v}"
        for v in ("weight", "bias"):
            k[f"conv{s}.{v}"] = f"conv{s}.{v}"
        for l in range(SWIN_LAYERS):
            for b in range(cfg["swin_depth"]):
                block(f"swin{s}.{l}.{b}.", f"swintransformer{s}.layers.{l}.blocks.{b}.", True)
    for ours, theirs in (("score", "fc_score"), ("weight", "fc_weight")):
        for v in ("weight", "bias"):
            k[f"{ours}.fc1.{v}"] = f"{theirs}.0.{v}"
            k[f"{ours}.fc2.{v}"] = f"{theirs}.3.{v}"
    return k


PYIQA_KEYS = _pyiqa_keys


def uniform_origins(h: int, w: int, crop: int, crops: int):
    """RECALLED FROM PYIQA (uniform_crop), unpinned: [(y, x)] - a grid of ceil(sqrt(crops)) positions per axis at the integer step
    (side - crop) // floor(sqrt(crops)), y outer, x inner, the first `crops` of them."""
    lo, hi = math.isqrt(crops), math.isqrt(crops - 1) + 1 if crops > 1 else 1
    sh, sw = (h - crop) // lo, (w - crop) // lo
    return [(i * sh, j * sw) for i in range(hi) for j in range(hi)][:crops]


# ---------------------------------------------------------------------------------------------------------------- input and crops
def scaled_input(img8) -> torch.Tensor:
    """[3][h][w] float32: step 1 of an HWC uint8 image."""
    x = torch.from_numpy(np.asarray(img8, np.float32) / np.float32(255.0)).permute(2, 0, 1)
    x = (x - np.float32(0.5)) / np.float32(0.5)
    assert x.dtype == torch.float32
    return x


def input_table() -> np.ndarray:
    """[256] float32: step 1 of every byte, by torch's float32 roundings."""
    v = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(3, axis=2)
    return scaled_input(v)[0, :, 0].numpy().copy()


def crop_origins(h: int, w: int, crop: int, crops: int, mode: str = "uniform", seed=None, name=None):
    """[(y, x)] * crops, step 2. mode "random": every origin uniform over the valid range, from a generator keyed by `seed` (DEFAULT_SEED when
    None) and the crc32 of the file's NAME - neither the order of the files nor the sharding over ranks moves a score."""
    if min(h, w) <= crop:
        raise ManiqaError(f"a {h} x {w} image has no {crop} x {crop} crops (the short side must be above {crop})")
    if crops < 1:
        raise ManiqaError(f"{crops} crops")
    if mode == "uniform":
        return uniform_origins(h, w, crop, crops)
    if mode != "random":
        raise ManiqaError(f"crop mode {mode!r} (uniform or random)")
    rng = np.random.default_rng([DEFAULT_SEED if seed is None else int(seed), zlib.crc32(str(name or "").encode())])
    ys, xs = rng.integers(0, h - crop + 1, crops), rng.integers(0, w - crop + 1, crops)
    return [(int(y), int(x)) for y, x in zip(ys, xs)]


def check_origins(h: int, w: int, crop: int, origins) -> None:
    for y, x in origins:
        if not (0 <= y <= h - crop and 0 <= x <= w - crop):
            raise ManiqaError(f"the crop origin ({y}, {x}) leaves a {h} x {w} image (crop {crop})")


# ---------------------------------------------------------------------------------------------------------------- the model's parts
def tab_reinterpret(p: torch.Tensor) -> torch.Tensor:
    """Step 4's reinterpretation of the product P [C][N]: out.flat[n * C + c] = P[c][n]."""
    C, N = p.shape
    return p.transpose(0, 1).reshape(C, N)


def relative_position_index(ws: int, transposed: bool = False) -> torch.Tensor:
    """[ws^2][ws^2] int64, as Swin builds it."""
    co = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0) + (ws - 1)
    idx = rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]
    return idx.t().contiguous() if transposed else idx


def shift_mask(G: int, ws: int, shift: int) -> torch.Tensor:
    """[windows][ws^2][ws^2] float64: 0 or MASK, as Swin builds it from the region labels of the shifted map."""
    img = torch.zeros((G, G))
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    mw = img.reshape(G // ws, ws, G // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    d = mw[:, None, :] - mw[:, :, None]
    return torch.where(d != 0, torch.tensor(MASK, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))


def _lin(x, sd, name, dt):
    return F.linear(x, sd[name + ".weight"].to(dt), sd[name + ".bias"].to(dt))


def _ln(x, sd, name, eps, dt):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"].to(dt), sd[name + ".bias"].to(dt), eps)


def _gelu(x, variant):
    return F.gelu(x, approximate="tanh" if variant == "gelu_tanh" else "none")


def vit_taps(x: torch.Tensor, model, variant=None) -> torch.Tensor:
    """Step 3: [B][N or 1 + N][4 embed] of the crops [B][3][crop][crop]."""
    sd, cfg, dt = model["sd"], model["cfg"], x.dtype
    E, heads, p = cfg["embed"], cfg["vit_heads"], cfg["patch"]
    hd = E // heads
    eps = 1e-5 if variant == "vit_ln_eps_1e5" else VIT_LN_EPS
    t = F.conv2d(x, sd["vit.patch.weight"].to(dt), sd["vit.patch.bias"].to(dt), stride=p).flatten(2).transpose(1, 2)
    B = t.shape[0]
    t = torch.cat([sd["vit.cls_token"].to(dt)[None, None].expand(B, 1, E), t], 1) + sd["vit.pos_embed"].to(dt)[None]
    T = t.shape[1]
    taps = [k - 1 for k in cfg["taps"]] if variant == "taps_shifted" else list(cfg["taps"])
    out = {}
    for i in range(max(taps) + 1):
        b = f"vit.blocks.{i}."
        q, k, v = _lin(_ln(t, sd, b + "ln1", eps, dt), sd, b + "attn.qkv", dt).reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1)
        t = t + _lin((a @ v).transpose(1, 2).reshape(B, T, E), sd, b + "attn.proj", dt)
        t = t + _lin(_gelu(_lin(_ln(t, sd, b + "ln2", eps, dt), sd, b + "mlp.fc1", dt), variant), sd, b + "mlp.fc2", dt)
        out[i] = t
    if variant == "taps_keep_cls":   # the class token kept, the last patch token lost: the shapes stay
        return torch.cat([out[i][:, :-1] for i in taps], 2)
    return torch.cat([out[i][:, 1:] for i in taps], 2)


def tab(x: torch.Tensor, sd, name, variant=None) -> torch.Tensor:
    """Step 4 on x [B][C][N]."""
    dt = x.dtype
    B, C, N = x.shape
    q, k, v = (_lin(x, sd, f"{name}.{n}", dt) for n in "qkv")
    a = (q @ k.transpose(-2, -1)) * (C if variant == "tab_scale_c" else N) ** -0.5
    a = torch.softmax(a, dim=-2 if variant == "tab_softmax_axis" else -1)
    p = a @ v
    if variant != "tab_transposed_back":
        p = p.transpose(1, 2).reshape(B, C, N)
    return p + x


def swin_block(x: torch.Tensor, sd, name, G, ws, heads, shift, variant=None) -> torch.Tensor:
    """One block of step 6 on the tokens x [B][G * G][D]."""
    dt = x.dtype
    B, L, D = x.shape
    hd, nw, W = D // heads, G // ws, ws * ws
    h = _ln(x, sd, name + "ln1", SWIN_LN_EPS, dt).reshape(B, G, G, D)
    if shift:
        h = torch.roll(h, (-shift, -shift), (1, 2))
    h = h.reshape(B, nw, ws, nw, ws, D).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, W, D)
    q, k, v = _lin(h, sd, name + "attn.qkv", dt).reshape(-1, W, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = (q * hd ** -0.5) @ k.transpose(-1, -2)
    idx = relative_position_index(ws, variant == "rpb_index_transposed")
    a = a + sd[name + "attn.rpb"].to(dt)[idx.reshape(-1)].reshape(W, W, heads).permute(2, 0, 1)[None]
    if shift and variant != "no_shift_mask":
        a = (a.reshape(B, nw * nw, heads, W, W) + shift_mask(G, ws, shift).to(dt)[None, :, None]).reshape(-1, heads, W, W)
    h = _lin((torch.softmax(a, dim=-1) @ v).transpose(1, 2).reshape(-1, W, D), sd, name + "attn.proj", dt)
    h = h.reshape(B, nw, nw, ws, ws, D).permute(0, 1, 3, 2, 4, 5).reshape(B, G, G, D)
    if shift:
        h = torch.roll(h, (shift, shift), (1, 2))
    x = x + h.reshape(B, L, D)
    return x + _lin(_gelu(_lin(_ln(x, sd, name + "ln2", SWIN_LN_EPS, dt), sd, name + "mlp.fc1", dt), variant), sd, name + "mlp.fc2", dt)


def swin_stage(x: torch.Tensor, model, s: int, variant=None) -> torch.Tensor:
    cfg = model["cfg"]
    G, ws = cfg["crop"] // cfg["patch"], cfg["window"]
    for l in range(SWIN_LAYERS):
        y = x
        for b in range(cfg["swin_depth"]):
            y = swin_block(y, model["sd"], f"swin{s}.{l}.{b}.", G, ws, cfg["swin_heads"], ws // 2 if b % 2 else 0, variant)
        x = y + x if variant == "no_scale" else cfg["scale"] * y + x
    return x


def crop_tokens(x: torch.Tensor, model, variant=None) -> torch.Tensor:
    """Steps 3 - 6: the tokens [B][N][embed / 2] the two heads read, of the crops [B][3][crop][crop]."""
    sd, dt = model["sd"], x.dtype
    t = vit_taps(x, model, variant).transpose(1, 2)                       # [B][C][N]
    for s in (1, 2):
        for k in range(TABS):
            t = tab(t, sd, f"tab{s}.{k}", variant)
        t = torch.einsum("oc,bcn->bno", sd[f"conv{s}.weight"].to(dt), t) + sd[f"conv{s}.bias"].to(dt)
        t = swin_stage(t, model, s, variant)
        if s == 1:
            t = t.transpose(1, 2)
    return t


def heads(t: torch.Tensor, sd):
    """Step 7's per-patch (s, w) of the tokens [...][embed / 2]."""
    dt = t.dtype
    s = F.relu(_lin(F.relu(_lin(t, sd, "score.fc1", dt)), sd, "score.fc2", dt))[..., 0]
    w = torch.sigmoid(_lin(F.relu(_lin(t, sd, "weight.fc1", dt)), sd, "weight.fc2", dt))[..., 0]
    return s, w


def score_image(img8, model, origins=None, dtype=torch.float32, variant=None, chunk: int = 4):
    """(score as a float, the head-input tokens [crops][N][embed / 2] as an array in dtype, (s, w) [crops][N] each) of one HWC uint8 image at
    the crop origins [(y, x)] (None: the uniform grid of the model's crop count)."""
    img8 = np.asarray(img8)
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise ManiqaError(f"an HWC uint8 RGB array is needed, got {img8.shape} {img8.dtype}")
    cfg = model["cfg"]
    h, w, crop = img8.shape[0], img8.shape[1], cfg["crop"]
    if origins is None:
        origins = crop_origins(h, w, crop, cfg["crops"])
    if min(h, w) <= crop:
        raise ManiqaError(f"a {h} x {w} image has no {crop} x {crop} crops (the short side must be above {crop})")
    check_origins(h, w, crop, origins)
    if variant == "origins_swapped":
        origins = [(min(x, h - crop), min(y, w - crop)) for y, x in origins]
    with torch.no_grad():
        x = scaled_input(img8).to(dtype)
        cr = torch.stack([x[:, oy:oy + crop, ox:ox + crop] for oy, ox in origins])
        tok = torch.cat([crop_tokens(cr[i:i + chunk], model, variant) for i in range(0, len(origins), chunk)])
        s, wt = heads(tok, model["sd"])
        s, wt = s.double(), wt.double()
        if variant == "per_crop_mean":
            score = ((wt * s).sum(1) / (wt.sum(1) + POOL_EPS)).mean()
        else:
            score = (wt * s).sum() / (wt.sum() + POOL_EPS)
    return float(score), tok.numpy(), (s.numpy(), wt.numpy())


def maniqa(img8, model, origins=None, dtype=torch.float32, variant=None) -> float:
    return score_image(img8, model, origins, dtype, variant)[0]


# ---------------------------------------------------------------------------------------------------------------- loading
def model_keys(cfg) -> dict:
    """{name: shape} of the model's tensors in the project's own names."""
    E, M, p, ws = cfg["embed"], cfg["vit_mlp"], cfg["patch"], cfg["window"]
    N = (cfg["crop"] // p) ** 2
    out = {"vit.patch.weight": (E, 3, p, p), "vit.patch.bias": (E,), "vit.cls_token": (E,), "vit.pos_embed": (1 + N, E)}

    def block(a, D, mlp, heads=None):
        for n, shape in (("ln1", None), ("ln2", None), ("attn.qkv", (3 * D, D)), ("attn.proj", (D, D)), ("mlp.fc1", (mlp, D)), ("mlp.fc2", (D, mlp))):
            out[a + n + ".weight"] = shape or (D,)
            out[a + n + ".bias"] = (shape[0],) if shape else (D,)
        if heads:
            out[a + "attn.rpb"] = ((2 * ws - 1) ** 2, heads)

    for i in range(cfg["vit_layers"]):
        block(f"vit.blocks.{i}.", E, M)
    for s, cin, D, mlp in ((1, 4 * E, E, cfg["dim_mlp"]), (2, E, E // 2, cfg["dim_mlp"] // 2)):
        for t in range(TABS):
            for n in "qkv":
                out[f"tab{s}.{t}.{n}.weight"], out[f"tab{s}.{t}.{n}.bias"] = (N, N), (N,)
        out[f"conv{s}.weight"], out[f"conv{s}.bias"] = (D, cin), (D,)
        for l in range(SWIN_LAYERS):
            for b in range(cfg["swin_depth"]):
                block(f"swin{s}.{l}.{b}.", D, mlp, cfg["swin_heads"])
    for n in ("score", "weight"):
        out[n + ".fc1.weight"], out[n + ".fc1.bias"], out[n + ".fc2.weight"], out[n + ".fc2.bias"] = (E // 2, E // 2), (E // 2,), (1, E // 2), (1,)
    return out


def config_of(sd, given=None) -> dict:
    """The configuration: the shapes from the tensors, the rest from `given` (cfg.* of an .npz, or the caller's dict) over DEFAULTS."""
    given = {**DEFAULTS, **(given or {})}
    try:
        E, p = int(sd["vit.patch.weight"].shape[0]), int(sd["vit.patch.weight"].shape[-1])
        N = int(sd["vit.pos_embed"].shape[-2]) - 1
        M = int(sd["vit.blocks.0.mlp.fc1.weight"].shape[0])
        dim_mlp = int(sd["swin1.0.0.mlp.fc1.weight"].shape[0])
        window = (int(round(math.sqrt(int(sd["swin1.0.0.attn.rpb"].shape[0])))) + 1) // 2
    except KeyError as e:
        raise ManiqaError(f"no MANIQA model: {e.args[0]} missing") from None
    G = math.isqrt(N)
    depth = 0
    while f"swin1.0.{depth}.ln1.weight" in sd:
        depth += 1
    taps = tuple(int(t) for t in given["taps"])
    if G * G != N or len(taps) != 4 or list(taps) != sorted(set(taps)) or taps[0] < 0:
        raise ManiqaError(f"no MANIQA model: {N} patch tokens, taps {taps}")
    return dict(crop=G * p, patch=p, embed=E, vit_heads=int(given["vit_heads"]), vit_mlp=M, vit_layers=taps[-1] + 1, taps=taps, window=window,
                swin_heads=int(given["swin_heads"]), swin_depth=depth, dim_mlp=dim_mlp, scale=float(given["scale"]), crops=int(given["crops"]))


def _read(path):
    """({name: float32 tensor} in the project's names, the given configuration values) of an .npz or of a .pth state dict."""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            sd = {k: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if not k.startswith("cfg.")}
            given = {k[4:]: (z[k].tolist() if z[k].ndim else z[k].item()) for k in z.files if k.startswith("cfg.")}
        return sd, given
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    for wrap in ("params", "state_dict"):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    if not isinstance(sd, dict):
        raise ManiqaError(f"{path}: no state dict")
    sd = {k: v.detach().float() for k, v in sd.items() if torch.is_tensor(v)}
    depth = 0
    while f"swintransformer1.layers.0.blocks.{depth}.norm1.weight" in sd:
        depth += 1
    out = {}
    for ours, theirs in PYIQA_KEYS(dict(vit_layers=DEFAULTS["taps"][-1] + 1, swin_depth=depth)).items():
        if theirs in sd:
            v = sd[theirs]
            out[ours] = v.reshape(-1) if ours == "vit.cls_token" else v.reshape(v.shape[-2:]) if ours == "vit.pos_embed" else \
                v.reshape(v.shape[:2]) if ours in ("conv1.weight", "conv2.weight") else v
    return out, {}


def load_model(path, cfg=None) -> dict:
    """{sd: the tensors in the project's names (float32), cfg}. path: an .npz, a .pth, or a dict in the project's names; cfg: values that the
    shapes do not fix (taps, scale, crops, vit_heads, swin_heads) over the file's own and DEFAULTS. A missing tensor or another shape raises
    ManiqaError naming it."""
    if isinstance(path, dict):
        sd, given = {k: torch.as_tensor(v).detach().float() for k, v in path.items()}, {}
    else:
        sd, given = _read(path)
    what = "the state dict" if isinstance(path, dict) else str(path)
    try:
        cfg = config_of(sd, {**given, **(cfg or {})})
    except ManiqaError as e:
        raise ManiqaError(f"{what}: {e}") from None
    E = cfg["embed"]
    if E % cfg["vit_heads"] or (E // 2) % cfg["swin_heads"] or (cfg["crop"] // cfg["patch"]) % cfg["window"]:
        raise ManiqaError(f"{what}: embed {E} with {cfg['vit_heads']} / {cfg['swin_heads']} heads, window {cfg['window']}")
    for k, shape in model_keys(cfg).items():
        if k not in sd:
            raise ManiqaError(f"{what}: {k} missing")
        if tuple(sd[k].shape) != shape:
            raise ManiqaError(f"{what}: {k} is {tuple(sd[k].shape)}, MANIQA of embed {E} has {shape}")
    return dict(sd={k: sd[k].contiguous() for k in model_keys(cfg)}, cfg=cfg)


def save_npz(path, model) -> None:
    cfg = model["cfg"]
    extra = {"cfg." + k: np.asarray(cfg[k]) for k in ("scale", "crops", "taps", "vit_heads", "swin_heads")}
    np.savez(path, **{k: v.numpy() for k, v in model["sd"].items()}, **extra)


# ---------------------------------------------------------------------------------------------------------------- the folder scorer
def evaluate(img_dir, model_path, ntest=None, backend="host", mode="uniform", seed=None, log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    model = load_model(model_path)
    cfg = model["cfg"]
    ctx = mq = None
    if backend == "gpu":
        if _ROOT not in sys.path:
            sys.path.insert(0, _ROOT)
        from instarevive_amd import _lib as L, maniqa as mq
        ctx = L.Context(0)
        mq.configure(ctx, model)
    total, scored, skipped = 0.0, 0, 0
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            org = crop_origins(img.shape[0], img.shape[1], cfg["crop"], cfg["crops"], mode, seed, f.name)
            v = mq.score_arrays(ctx, img, org) if ctx is not None else maniqa(img, model, org)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"maniqa: {total / scored:.5f}")
    return total / scored if scored else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--maniqa_model", required=True, help="the MANIQA koniq weights: an .npz in this file's names, or pyiqa's .pth")
    ap.add_argument("--maniqa_crops", choices=("uniform", "random"), default="uniform")
    ap.add_argument("--maniqa_seed", type=int, default=None, help=f"with --maniqa_crops random (default {DEFAULT_SEED})")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    try:
        evaluate(a.img_path, a.maniqa_model, a.ntest, backend=a.backend, mode=a.maniqa_crops, seed=a.maniqa_seed)
    except ManiqaError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    main()
