#!/usr/bin/env python3
"""MUSIQ of an output folder: the no-reference metric `musiq` of the reference's evaluate_img.py (`create_metric('musiq')`).

    python tools/evaluate_musiq.py -i results/ --musiq_model musiq_koniq.npz [--ntest N] [--backend gpu]

The reference takes it from pyiqa, which is not in this image, and the pretrained checkpoint does not exist offline either: the user passes it.
So the definition is RESTATED here as a plain torch model from the published implementation (pyiqa's `musiq`, default koniq10k configuration) -
parity with pyiqa itself is unpinned until a box that has it runs tools/repin_with_diffusers.py. Three things are recollections of pyiqa and
stand in one named place each, so that such a box can correct them in one spot: PYIQA_KEYS (the checkpoint's key names), standardize() (the
weight standardisation) and resize() (the resize call). This file is the model ir_musiq (csrc/musiq.hip) is tested against; it runs on the CPU
in float32 or float64. The metric is exact fp32 - evaluate_img.py's autocast / fp16 scoring is not reproduced.

  1. input: RGB bytes v; x = (v / 255 - 0.5) * 2 in float32, each step rounded in that order (a 256-entry table for all three channels).
  2. three scales with ids 0, 1, 2. Ids 0 and 1: the longer side becomes L = 224 / 384: ratio = L / max(h, w) in double, rh = round(h * ratio),
     rw = round(w * ratio) with Python's round (half to even), resize() = torch's bicubic (A = -0.75, align_corners=False, clamped taps, no
     antialias; small images are enlarged). Id 2: the image at its own size, every patch kept.
  3. patches: 32 x 32 at stride 32, TensorFlow 'SAME' padding per scale (count = ceil(size / 32), pad = count * 32 - size, pad // 2 in front),
     the pad value 0 in step 1's domain; a patch is flattened (c, y, x). pyiqa pads the two resized scales to 49 and 144 tokens with masked zero
     tokens: a masked key gets the score -1e3 and thus the weight exactly 0, and a masked query's output feeds nothing that reaches the class
     token - so this model (and the device) leaves those tokens out; padding="masked" keeps them, and the tests show that it is the same number.
     T = 1 + sum count_h * count_w.
  4. hashed spatial index of patch (i, j) of a count_h x count_w grid: hi * 10 + wj, hi = floor(i * (10 / count_h)) with the factor in float32
     (torch's nearest interpolation of arange(10)), wj likewise.
  5. patch stem (per patch, NCHW): weight-standardised conv 7 x 7 / 2, 3 -> 64, no bias, 'SAME' (2 in front, 3 behind: 32 -> 16);
     GroupNorm(32, eps 1e-6); ReLU; MaxPool 3 x 3 / 2 'SAME' (0 in front, 1 behind: 16 -> 8); one bottleneck - std-conv 1 x 1 64 -> 64,
     GroupNorm(32, eps 1e-4), ReLU; std-conv 3 x 3 'SAME' 64 -> 64, GroupNorm, ReLU; std-conv 1 x 1 64 -> 256, GroupNorm; projection branch
     std-conv 1 x 1 64 -> 256, GroupNorm; ReLU(out + projection). standardize(): (w - mean) / sqrt(var + 1e-5) per output channel, biased
     variance, in float64, rounded to float32 once when the model is loaded; the float32 and float64 models and the device read those weights.
     Flatten (y, x, c) to 16384 values, Linear 16384 -> 384.
  6. transformer input: + position_emb[index] (100 x 384), + scale_emb[scale id] (3 x 384); the class token in front.
  7. 14 pre-LN blocks, LayerNorm eps 1e-6: x += out(attn(LN1 x)) - six heads of 64, separate q / k / v / out linears with bias, scores scaled
     by 64^-0.5, softmax over all T keys; x += fc2(gelu(fc1(LN2 x))), the exact (erf) GELU, 384 -> 1152 -> 384.
  8. head: the final LayerNorm (eps 1e-6) of the class token, Linear 384 -> 1 with bias. That is the score (roughly 0 - 100 with the real
     weights; no clamp).
An image for which a resized side rounds to 0 (1 x 1000) is refused (MusiqError).

The model file: an .npz in the project's own names - the form that always works -
    stem.conv.weight [64][3][7][7], stem.gn.{weight,bias}; block.conv1.weight [64][64][1][1], block.gn1.*, block.conv2.weight [64][64][3][3],
    block.gn2.*, block.conv3.weight [256][64][1][1], block.gn3.*, block.proj.weight [256][64][1][1], block.gn_proj.*  (the RAW conv weights);
    embedding.{weight,bias} [384][16384]; position_emb [100][384]; scale_emb [3][384]; cls_token [384];
    layers.L.ln1.*, layers.L.attn.{q,k,v,out}.{weight,bias}, layers.L.ln2.*, layers.L.mlp.fc1.* [1152][384], layers.L.mlp.fc2.* [384][1152];
    final_ln.*; head.weight [1][384], head.bias [1]
or a torch .pth state dict (plain, or under `params` / `state_dict`) through PYIQA_KEYS.
Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import math
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

PATCH = 32
GRID = 10
LONGER = (224, 384, 0)        # the longer side of each scale; 0: the image at its own size
MAX_TOKENS = (49, 144, None)  # pyiqa pads a resized scale to this many tokens (padding="masked" / "unmasked")
STEM_GN_EPS, BLOCK_GN_EPS, LN_EPS, STD_EPS = 1e-6, 1e-4, 1e-6, 1e-5
BICUBIC_A = -0.75
CONVS = ("stem.conv", "block.conv1", "block.conv2", "block.conv3", "block.proj")
# what a wrong implementation might do instead, one per step; the tests show that the gate tells each apart
VARIANTS = ("stem_same_reversed", "pool_pad_front", "gn_eps_1e5", "unbiased_std", "flatten_cyx", "index_round", "no_scale_emb", "no_cls_token", "post_ln",
            "gelu_tanh", "pad_tokens_unmasked", "round_half_away", "bicubic_a05")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class MusiqError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- recollections of pyiqa (unpinned)
def standardize(w: torch.Tensor, unbiased: bool = False) -> torch.Tensor:
    """RECALLED FROM PYIQA (StdConv), unpinned: the weight standardisation, a function of the weights alone - (w - mean) / sqrt(var + 1e-5) per
    output channel with the biased variance, in float64, rounded to float32 once."""
    w = w.double()
    mean = w.mean(dim=(1, 2, 3), keepdim=True)
    var = w.var(dim=(1, 2, 3), keepdim=True, unbiased=unbiased)
    return ((w - mean) / torch.sqrt(var + STD_EPS)).float()


def resize(x: torch.Tensor, rh: int, rw: int) -> torch.Tensor:
    """RECALLED FROM PYIQA, unpinned: the resize call of the two smaller scales."""
    return F.interpolate(x, (rh, rw), mode="bicubic", align_corners=False)


def _pyiqa_keys(layers: int) -> dict:
    """RECALLED FROM PYIQA (musiq_arch.MUSIQ), unpinned: {this project's name: the checkpoint's key}."""
    k = {"stem.conv.weight": "conv_root.weight", "stem.gn.weight": "gn_root.weight", "stem.gn.bias": "gn_root.bias",
         "block.conv1.weight": "block1.unit01.conv1.weight", "block.gn1.weight": "block1.unit01.gn1.weight", "block.gn1.bias": "block1.unit01.gn1.bias",
         "block.conv2.weight": "block1.unit01.conv2.weight", "block.gn2.weight": "block1.unit01.gn2.weight", "block.gn2.bias": "block1.unit01.gn2.bias",
         "block.conv3.weight": "block1.unit01.conv3.weight", "block.gn3.weight": "block1.unit01.gn3.weight", "block.gn3.bias": "block1.unit01.gn3.bias",
         "block.proj.weight": "block1.unit01.conv_proj.weight", "block.gn_proj.weight": "block1.unit01.gn_proj.weight", "block.gn_proj.bias": "block1.unit01.gn_proj.bias",
         "embedding.weight": "embedding.weight", "embedding.bias": "embedding.bias",
         "position_emb": "transformer_encoder.posembed_input.position_emb", "scale_emb": "transformer_encoder.scaleembed_input.scale_emb",
         "cls_token": "transformer_encoder.cls", "final_ln.weight": "transformer_encoder.encoder_norm.weight", "final_ln.bias": "transformer_encoder.encoder_norm.bias",
         "head.weight": "head.weight", "head.bias": "head.bias"}
    for i in range(layers):
        a, b = f"layers.{i}.", f"transformer_encoder.encoderblock_{i:02d}."
        for v in ("weight", "bias"):
            k[f"{a}ln1.{v}"] = f"{b}layernorm1.{v}"
            k[f"{a}ln2.{v}"] = f"{b}layernorm2.{v}"
            for ours, theirs in (("q", "query"), ("k", "key"), ("v", "value"), ("out", "out")):
                k[f"{a}attn.{ours}.{v}"] = f"{b}attention.{theirs}.{v}"
            k[f"{a}mlp.fc1.{v}"] = f"{b}mlpblock.fc1.{v}"
            k[f"{a}mlp.fc2.{v}"] = f"{b}mlpblock.fc2.{v}"
    return k


PYIQA_KEYS = _pyiqa_keys


# ---------------------------------------------------------------------------------------------------------------- input and layout
def scaled_input(img8) -> torch.Tensor:
    """[1][3][h][w] float32: step 1 of an HWC uint8 image."""
    x = torch.from_numpy(np.asarray(img8, np.float32) / np.float32(255.0)).permute(2, 0, 1)[None]
    x = (x - np.float32(0.5)) * np.float32(2.0)
    assert x.dtype == torch.float32
    return x


def input_table() -> np.ndarray:
    """[256] float32: step 1 of every byte, by torch's float32 roundings."""
    v = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(3, axis=2)
    return scaled_input(v)[0, 0, :, 0].numpy().copy()


def _round_half_away(v: float) -> int:
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def hashed_axis(count: int, grid: int = GRID, rounded: bool = False) -> torch.Tensor:
    """[count] int64: torch's nearest interpolation of arange(grid) to count entries - floor(i * (grid / count)) with the factor in float32."""
    if rounded:
        return torch.tensor([min(_round_half_away(i * grid / count), grid - 1) for i in range(count)], dtype=torch.int64)
    return F.interpolate(torch.arange(grid, dtype=torch.float32)[None, None], size=count, mode="nearest")[0, 0].long()


def layout(h: int, w: int, variant=None, longer=LONGER, grid: int = GRID):
    """(scales, index, T): per scale (rh, rw, count_h, count_w, pad_top, pad_left) - steps 2 and 3 - and the hashed spatial index of every patch
    token in token order (scale by scale, row by row) - step 4. MusiqError when a resized side rounds to 0."""
    rnd = _round_half_away if variant == "round_half_away" else round
    scales, index = [], []
    for L in longer:
        rh, rw = h, w
        if L:
            ratio = L / max(h, w)
            rh, rw = int(rnd(h * ratio)), int(rnd(w * ratio))
            if rh < 1 or rw < 1:
                raise MusiqError(f"a resized side of a {h} x {w} image rounds to 0 (longer side {L})")
        ch, cw = -(-rh // PATCH), -(-rw // PATCH)
        scales.append((rh, rw, ch, cw, (ch * PATCH - rh) // 2, (cw * PATCH - rw) // 2))
        hi, wj = hashed_axis(ch, grid, variant == "index_round"), hashed_axis(cw, grid, variant == "index_round")
        index.append((hi[:, None] * grid + wj[None, :]).reshape(-1))
    index = torch.cat(index)
    return scales, index, 1 + int(index.numel())


def bicubic(x: torch.Tensor, rh: int, rw: int, A: float = BICUBIC_A) -> torch.Tensor:
    """resize() written out, in x's dtype: source coordinate (in / out) * (dst + 0.5) - 0.5, four taps per axis clamped to the image, the cubic
    convolution weights of parameter A. Serves the variant with another A; with A = -0.75 in float64 it equals resize()."""
    def axis(n_in, n_out):
        src = (n_in / n_out) * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5
        f = torch.floor(src)
        t = src - f
        c = torch.stack([((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                         ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1, ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A], dim=1)
        taps = (f.long()[:, None] + torch.arange(-1, 3)[None]).clamp(0, n_in - 1)
        return taps, c.to(x.dtype)

    ty, cy = axis(x.shape[2], rh)
    tx, cx = axis(x.shape[3], rw)
    rows = (x[:, :, :, tx] * cx).sum(-1)                                   # [n][c][h][rw]
    return (rows[:, :, ty, :] * cy[None, None, :, :, None]).sum(3)       # [n][c][rh][rw]


def patches_of(x: torch.Tensor, variant=None, padding="drop", longer=LONGER):
    """(patches [P][3][32][32] in x's dtype, index [P], scale id [P], mask [P] bool) of the scaled input [1][3][h][w]: steps 2 - 4. padding: "drop"
    leaves pyiqa's padding tokens of the resized scales out; "masked" / "unmasked" append them (zero pixels, index 0) with mask False."""
    h, w = x.shape[2:]
    scales, index, _ = layout(h, w, variant, longer)
    out, idx, sid, mask, at = [], [], [], [], 0
    for s, (rh, rw, ch, cw, pt, pl) in enumerate(scales):
        xs = x
        if longer[s]:
            xs = bicubic(x, rh, rw, -0.5) if variant == "bicubic_a05" else resize(x, rh, rw)
        xs = F.pad(xs, (pl, cw * PATCH - rw - pl, pt, ch * PATCH - rh - pt))
        p = xs[0].reshape(3, ch, PATCH, cw, PATCH).permute(1, 3, 0, 2, 4).reshape(ch * cw, 3, PATCH, PATCH)
        k = ch * cw
        i = index[at:at + k]
        at += k
        extra = (MAX_TOKENS[s] - k) if (padding != "drop" and s < len(MAX_TOKENS) and MAX_TOKENS[s]) else 0
        if extra > 0:
            p = torch.cat([p, torch.zeros((extra, 3, PATCH, PATCH), dtype=x.dtype)])
            i = torch.cat([i, torch.zeros(extra, dtype=torch.int64)])
        out.append(p)
        idx.append(i)
        sid.append(torch.full((p.shape[0],), s, dtype=torch.int64))
        mask.append(torch.cat([torch.ones(k, dtype=torch.bool), torch.zeros(max(extra, 0), dtype=torch.bool)]))
    return torch.cat(out), torch.cat(idx), torch.cat(sid), torch.cat(mask)


# ---------------------------------------------------------------------------------------------------------------- the model
def patch_stem(p: torch.Tensor, model, variant=None) -> torch.Tensor:
    """Step 5: [P][384] of the patches [P][3][32][32], in p's dtype."""
    dt = p.dtype
    sd = model["sd"]

    def t(key):
        return sd[key].to(dt)

    def conv(x, name, stride=1, pad=0):
        w = standardize(sd[name + ".weight"], unbiased=True) if variant == "unbiased_std" else model["std"][name]
        return F.conv2d(x, w.to(dt), None, stride, pad)

    def gn(x, name, eps):
        return F.group_norm(x, 32, t(name + ".weight"), t(name + ".bias"), 1e-5 if variant == "gn_eps_1e5" else eps)

    x = conv(F.pad(p, (3, 2, 3, 2) if variant == "stem_same_reversed" else (2, 3, 2, 3)), "stem.conv", 2)
    x = F.relu(gn(x, "stem.gn", STEM_GN_EPS))
    x = F.max_pool2d(F.pad(x, (1, 0, 1, 0) if variant == "pool_pad_front" else (0, 1, 0, 1), value=float("-inf")), 3, 2)
    y = F.relu(gn(conv(x, "block.conv1"), "block.gn1", BLOCK_GN_EPS))
    y = F.relu(gn(conv(y, "block.conv2", 1, 1), "block.gn2", BLOCK_GN_EPS))
    y = gn(conv(y, "block.conv3"), "block.gn3", BLOCK_GN_EPS)
    x = F.relu(y + gn(conv(x, "block.proj"), "block.gn_proj", BLOCK_GN_EPS))
    x = x.reshape(x.shape[0], -1) if variant == "flatten_cyx" else x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    return F.linear(x, t("embedding.weight"), t("embedding.bias"))


def transformer(tok: torch.Tensor, mask, model, variant=None):
    """Steps 7 and 8 on the tokens [T][384] (the class token first, unless the variant drops it): (score, the final LayerNorm of token 0).
    mask: None, or [T] bool - a False key gets the score -1e3."""
    dt = tok.dtype
    sd, cfg = model["sd"], model["cfg"]
    heads, C = cfg["heads"], cfg["hidden"]
    hd = C // heads

    def t(key):
        return sd[key].to(dt)

    def lin(x, name):
        return F.linear(x, t(name + ".weight"), t(name + ".bias"))

    def ln(x, name):
        return F.layer_norm(x, (C,), t(name + ".weight"), t(name + ".bias"), LN_EPS)

    def attn(x, p):
        T = x.shape[0]
        q, k, v = (lin(x, p + "attn." + n).view(T, heads, hd).transpose(0, 1) for n in ("q", "k", "v"))
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        if mask is not None:
            s = s.masked_fill(~mask[None, None, :], -1e3)
        return lin((torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(T, C), p + "attn.out")

    def mlp(x, p):
        return lin(F.gelu(lin(x, p + "mlp.fc1"), approximate="tanh" if variant == "gelu_tanh" else "none"), p + "mlp.fc2")

    x = tok
    for i in range(cfg["layers"]):
        p = f"layers.{i}."
        if variant == "post_ln":
            x = ln(x + attn(x, p), p + "ln1")
            x = ln(x + mlp(x, p), p + "ln2")
        else:
            x = x + attn(ln(x, p + "ln1"), p)
            x = x + mlp(ln(x, p + "ln2"), p)
    feat = ln(x[0], "final_ln")
    return F.linear(feat, t("head.weight"), t("head.bias"))[0], feat


def score_image(img8, model, dtype=torch.float32, variant=None, padding="drop"):
    """(score as a float, the final-LN class token [384] as an array in dtype) of one HWC uint8 image."""
    img8 = np.asarray(img8)
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise MusiqError(f"an HWC uint8 RGB array is needed, got {img8.shape} {img8.dtype}")
    if variant == "pad_tokens_unmasked":
        padding = "unmasked"
    sd = model["sd"]
    with torch.no_grad():
        x = scaled_input(img8).to(dtype)
        p, idx, sid, mask = patches_of(x, variant, padding, model["cfg"]["longer"])
        tok = patch_stem(p, model, variant) + sd["position_emb"].to(dtype)[idx]
        if variant != "no_scale_emb":
            tok = tok + sd["scale_emb"].to(dtype)[sid]
        if variant != "no_cls_token":
            tok = torch.cat([sd["cls_token"].to(dtype)[None], tok])
            mask = torch.cat([torch.ones(1, dtype=torch.bool), mask])
        score, feat = transformer(tok, mask if padding == "masked" else None, model, variant)
    return float(score.double()), feat.numpy()


def musiq(img8, model, dtype=torch.float32, variant=None) -> float:
    return score_image(img8, model, dtype, variant)[0]


# ---------------------------------------------------------------------------------------------------------------- loading
def model_keys(cfg) -> dict:
    """{name: shape} of the model's tensors in the project's own names."""
    C, M = cfg["hidden"], cfg["mlp"]
    out = {"stem.conv.weight": (64, 3, 7, 7), "block.conv1.weight": (64, 64, 1, 1), "block.conv2.weight": (64, 64, 3, 3), "block.conv3.weight": (256, 64, 1, 1),
           "block.proj.weight": (256, 64, 1, 1), "embedding.weight": (C, 8 * 8 * 256), "embedding.bias": (C,), "position_emb": (cfg["grid"] ** 2, C),
           "scale_emb": (len(cfg["longer"]), C), "cls_token": (C,), "head.weight": (1, C), "head.bias": (1,)}
    for name, n in (("stem.gn", 64), ("block.gn1", 64), ("block.gn2", 64), ("block.gn3", 256), ("block.gn_proj", 256), ("final_ln", C)):
        out[name + ".weight"] = out[name + ".bias"] = (n,)
    for i in range(cfg["layers"]):
        p = f"layers.{i}."
        for name, shape in (("ln1", None), ("ln2", None), ("attn.q", (C, C)), ("attn.k", (C, C)), ("attn.v", (C, C)), ("attn.out", (C, C)), ("mlp.fc1", (M, C)),
                            ("mlp.fc2", (C, M))):
            out[p + name + ".weight"] = shape or (C,)
            out[p + name + ".bias"] = (shape[0],) if shape else (C,)
    return out


def config_of(sd) -> dict:
    try:
        C = int(sd["embedding.weight"].shape[0])
        M = int(sd["layers.0.mlp.fc1.weight"].shape[0])
    except KeyError as e:
        raise MusiqError(f"no MUSIQ model: {e.args[0]} missing") from None
    layers = 0
    while f"layers.{layers}.ln1.weight" in sd:
        layers += 1
    if C % 64:
        raise MusiqError(f"the hidden size {C} is no multiple of the head size 64")
    return dict(patch=PATCH, hidden=C, mlp=M, heads=C // 64, layers=layers, grid=GRID, longer=LONGER)


def _read(path) -> dict:
    """{name: float32 tensor} in the project's names, of an .npz in those names or of a .pth state dict (plain, or under params / state_dict)."""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(np.asarray(z[k])).float() for k in z.files}
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    for wrap in ("params", "state_dict"):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    if not isinstance(sd, dict):
        raise MusiqError(f"{path}: no state dict")
    sd = {k: v.detach().float() for k, v in sd.items() if torch.is_tensor(v)}
    layers = 0
    while PYIQA_KEYS(layers + 1)[f"layers.{layers}.ln1.weight"] in sd:
        layers += 1
    out = {}
    for ours, theirs in PYIQA_KEYS(layers).items():
        if theirs in sd:
            v = sd[theirs]
            out[ours] = v.reshape(v.shape[-2:]) if ours in ("position_emb", "scale_emb") else v.reshape(-1) if ours == "cls_token" else v
    return out


def load_model(path) -> dict:
    """{sd: the tensors in the project's names (float32, the raw conv weights), std: {conv name: the standardised weight}, cfg}. path: an .npz, a
    .pth, or a dict in the project's names. A missing tensor or another shape raises MusiqError naming it."""
    sd = _read(path) if not isinstance(path, dict) else {k: torch.as_tensor(v).detach().float() for k, v in path.items()}
    what = "the state dict" if isinstance(path, dict) else str(path)
    try:
        cfg = config_of(sd)
    except MusiqError as e:
        raise MusiqError(f"{what}: {e}") from None
    for k, shape in model_keys(cfg).items():
        if k not in sd:
            raise MusiqError(f"{what}: {k} missing")
        if tuple(sd[k].shape) != shape:
            raise MusiqError(f"{what}: {k} is {tuple(sd[k].shape)}, MUSIQ of hidden size {cfg['hidden']} has {shape}")
    sd = {k: sd[k].contiguous() for k in model_keys(cfg)}
    return dict(sd=sd, cfg=cfg, std={c: standardize(sd[c + ".weight"]) for c in CONVS})


def save_npz(path, model) -> None:
    np.savez(path, **{k: v.numpy() for k, v in model["sd"].items()})


# ---------------------------------------------------------------------------------------------------------------- the folder scorer
def evaluate(img_dir, model_path, ntest=None, backend="host", log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    model = load_model(model_path)
    ctx = mq = None
    if backend == "gpu":
        if _ROOT not in sys.path:
            sys.path.insert(0, _ROOT)
        from instarevive_amd import _lib as L, musiq as mq
        ctx = L.Context(0)
        mq.configure(ctx, model)
    total, scored, skipped = 0.0, 0, 0
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            v = mq.score_arrays(ctx, img) if ctx is not None else musiq(img, model)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"musiq: {total / scored:.5f}")
    return total / scored if scored else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--musiq_model", required=True, help="the MUSIQ koniq10k weights: an .npz in this file's names, or pyiqa's .pth")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    try:
        evaluate(a.img_path, a.musiq_model, a.ntest, backend=a.backend)
    except MusiqError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    main()
