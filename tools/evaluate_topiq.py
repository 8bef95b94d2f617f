#!/usr/bin/env python3
"""TOPIQ-NR of an output folder: the no-reference metric `topiq_nr` that the reference's evaluate_img.py names (commented out) next to its live
metrics.

    python tools/evaluate_topiq.py -i results/ --topiq_model topiq_nr.npz [--ntest N] [--backend gpu]

pyiqa, timm and the pretrained checkpoint do not exist offline: the user passes the weights, and the definition is RESTATED here as a plain
torch model from the published implementation (pyiqa's `CFANet` in the `topiq_nr` configuration: a timm `resnet50` trunk, use_ref=False, one
attention layer per stage, the image at its own size, no test-time resize). Parity with pyiqa itself is unpinned until a box that has it runs
tools/repin_with_diffusers.py (item 16). The recollections of pyiqa stand in one named place each: PYIQA_KEYS (the checkpoint's key names),
decoder_layer() (no self-attention in the coarse-to-fine layer - the loader refuses a checkpoint whose decoder layers carry `self_attn`
tensors instead of scoring another model) and DEFAULT_HEADS (a state dict's shapes do not hold the head count). This file is the model
ir_topiq (csrc/topiq.hip) is tested against; it runs on the CPU in float32 or float64, and its float64 run is the device's model.

  1. input: RGB bytes v; x = (v / 255 - mean) / std per channel in float32, each step rounded in that order (a 3 x 256 table, mean
     (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225)); padding is 0 in that domain.
  2. trunk: conv 7 x 7 / 2 / pad 3 without bias, BatchNorm, ReLU - feature 0 (width channels); MaxPool 3 x 3 / 2 / pad 1; four stages of
     bottlenecks (1 x 1; 3 x 3 carrying the stride; 1 x 1 to 4 x planes; a 1 x 1 projection shortcut with the stage's stride in a stage's first
     block), depths (3, 4, 6, 3), strides (1, 2, 2, 2) - features 1 .. 4 (4, 8, 16, 32 x width channels). BatchNorm is frozen, eps 1e-5, folded
     into scale = g / sqrt(var + eps), shift = b - mean scale in float64 and rounded to float32 once; both models and the device read those.
     Every strided size is floor((s - 1) / 2) + 1.
  3. per level i: GatedConv - splitconv 1 x 1 C -> 2 C chunked x1 | x2, w = sigmoid(conv3x3(64 -> 1)(gelu(conv3x3(64 -> 64)(gelu(conv1x1(C ->
     64)(x2)))))), out = gelu(x1) * w, erf GELU, zero padding, biases everywhere; adaptive_avg_pool2d to level 4's (th, tw) when the map's height
     AND width are both above it (bins floor(i H / th) .. ceil((i + 1) H / th)); dim_reduce 1 x 1 C -> D and GELU; + position_table();
     one pre-norm encoder layer (LN eps 1e-5; nn.MultiheadAttention's arithmetic: packed in_proj, q scaled by hd^-0.5 before q k^T, out_proj).
  4. position_table(): cat(h_emb repeated along x, w_emb repeated along y) on the channel axis, 32 x 32, interpolated to the map's size with
     torch's bicubic (align_corners=False, A = -0.75, clamped taps, no antialias) written out in float64 - x first, then y, each a four-term
     sum from the left - and rounded once to float32.
  5. coarse to fine: query = level 4's tokens; query = decoder_k(query, tokens of level 3 - k) for k = 0 .. 3; decoder_layer():
     m = LN2(memory), t = LN1(query), query += MHA(t, m, m), query += FFN(LN3(query)).
  6. attn_pool: one more encoder layer on the query; feat = the mean over its tokens; score_linear: LN, Linear, GELU, LN, Linear, GELU,
     Linear(D, 1). No output activation.
Images with a side below 16 are refused (TopiqError).

The model file: an .npz in the project's own names (model_keys(); optionally a scalar `heads`) or pyiqa's .pth (plain or under `params`)
through PYIQA_KEYS. Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import math
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BN_EPS, LN_EPS = 1e-5, 1e-5
BICUBIC_A = -0.75
GATE_HIDDEN = 64
EMB_SIZE = 32
MIN_EDGE = 16
STRIDES = (1, 2, 2, 2)
DEFAULT_HEADS = 4   # RECALLED FROM PYIQA (CFANet's num_attn_heads), unpinned: a state dict's shapes do not hold it
# what a wrong implementation might do instead; the tests show that the gate tells each apart
VARIANTS = ("stride_on_conv1", "pool_floor_end", "pool_or", "chunk_swapped", "gelu_tanh", "bicubic_a05", "pos_halves_swapped", "memory_not_normed",
            "query_memory_swapped", "fine_to_coarse", "post_norm", "mean_before_pool")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TopiqError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- names
def _attn_keys(ours: str, theirs: str, attn: str, norms: int) -> dict:
    k = {}
    for v in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
        k[f"{ours}attn.{v}"] = f"{theirs}{attn}.{v}"
    for name in ["linear1", "linear2"] + [f"norm{j + 1}" for j in range(norms)]:
        for v in ("weight", "bias"):
            k[f"{ours}{name}.{v}"] = f"{theirs}{name}.{v}"
    return k


def _conv_bn(conv: str, bn: str):
    return [conv + ".weight"] + [f"{bn}.{v}" for v in ("weight", "bias", "running_mean", "running_var")]


def trunk_convs(depths):
    """[(conv name, bn name, stage 0 .. 3 or -1 for the stem, block, which)] of the trunk in order."""
    out = [("trunk.conv1", "trunk.bn1", -1, 0, "stem")]
    for l, d in enumerate(depths):
        for b in range(d):
            p = f"trunk.layer{l + 1}.{b}."
            for j in (1, 2, 3):
                out.append((f"{p}conv{j}", f"{p}bn{j}", l, b, f"conv{j}"))
            if b == 0:
                out.append((f"{p}downsample.0", f"{p}downsample.1", l, b, "down"))
    return out


def _pyiqa_keys(depths) -> dict:
    """RECALLED FROM PYIQA (cfanet_arch.CFANet over timm's resnet50 feature net), unpinned: {this project's name: the checkpoint's key}."""
    k = {}
    for conv, bn, *_ in trunk_convs(depths):
        for name in _conv_bn(conv, bn):
            k[name] = "semantic_model." + name[len("trunk."):]
    for i in range(5):
        for ours, theirs in (("split", "splitconv"), ("conv1", "weight_blk.0"), ("conv2", "weight_blk.2"), ("conv3", "weight_blk.4")):
            for v in ("weight", "bias"):
                k[f"gate.{i}.{ours}.{v}"] = f"weight_pool.{i}.{theirs}.{v}"
        for v in ("weight", "bias"):
            k[f"reduce.{i}.{v}"] = f"dim_reduce.{i}.0.{v}"
        k.update(_attn_keys(f"sa.{i}.", f"sa_attn_blks.{i}.layers.0.", "self_attn", 2))
    for j in range(4):
        k.update(_attn_keys(f"ca.{j}.", f"attn_blks.{j}.layers.0.", "multihead_attn", 3))
    k.update(_attn_keys("pool.", "attn_pool.", "self_attn", 2))
    for j in (0, 1, 3, 4, 6):
        for v in ("weight", "bias"):
            k[f"score.{j}.{v}"] = f"score_linear.{j}.{v}"
    k["h_emb"] = "h_emb"
    k["w_emb"] = "w_emb"
    return k


PYIQA_KEYS = _pyiqa_keys


def model_keys(cfg) -> dict:
    """{name: shape} of the model's tensors in the project's own names."""
    W, D, Fn = cfg["width"], cfg["dim"], cfg["ffn"]
    out = {}
    inplanes = W
    for conv, bn, l, b, which in trunk_convs(cfg["depths"]):
        planes = W << max(l, 0)
        if which == "stem":
            shape = (W, 3, 7, 7)
        elif which == "conv1":
            shape = (planes, inplanes, 1, 1)
        elif which == "conv2":
            shape = (planes, planes, 3, 3)
        elif which == "conv3":
            shape = (4 * planes, planes, 1, 1)
        else:
            shape = (4 * planes, inplanes, 1, 1)
        if which == "conv3" and b > 0 or which == "down":
            inplanes = 4 * planes
        out[conv + ".weight"] = shape
        for v in ("weight", "bias", "running_mean", "running_var"):
            out[f"{bn}.{v}"] = (shape[0],)

    def attn(p, norms):
        out[p + "attn.in_proj_weight"] = (3 * D, D)
        out[p + "attn.in_proj_bias"] = (3 * D,)
        out[p + "attn.out_proj.weight"] = (D, D)
        out[p + "attn.out_proj.bias"] = (D,)
        out[p + "linear1.weight"] = (Fn, D)
        out[p + "linear1.bias"] = (Fn,)
        out[p + "linear2.weight"] = (D, Fn)
        out[p + "linear2.bias"] = (D,)
        for j in range(norms):
            out[f"{p}norm{j + 1}.weight"] = out[f"{p}norm{j + 1}.bias"] = (D,)

    for i, C in enumerate(level_channels(W)):
        g = f"gate.{i}."
        out[g + "split.weight"], out[g + "split.bias"] = (2 * C, C, 1, 1), (2 * C,)
        out[g + "conv1.weight"], out[g + "conv1.bias"] = (GATE_HIDDEN, C, 1, 1), (GATE_HIDDEN,)
        out[g + "conv2.weight"], out[g + "conv2.bias"] = (GATE_HIDDEN, GATE_HIDDEN, 3, 3), (GATE_HIDDEN,)
        out[g + "conv3.weight"], out[g + "conv3.bias"] = (1, GATE_HIDDEN, 3, 3), (1,)
        out[f"reduce.{i}.weight"], out[f"reduce.{i}.bias"] = (D, C, 1, 1), (D,)
        attn(f"sa.{i}.", 2)
    for j in range(4):
        attn(f"ca.{j}.", 3)
    attn("pool.", 2)
    for j, shape in ((0, (D,)), (1, (D, D)), (3, (D,)), (4, (D, D)), (6, (1, D))):
        out[f"score.{j}.weight"] = shape
        out[f"score.{j}.bias"] = (shape[0],)
    out["h_emb"] = (1, D // 2, EMB_SIZE, 1)
    out["w_emb"] = (1, D // 2, 1, EMB_SIZE)
    return out


def level_channels(width: int):
    return (width, 4 * width, 8 * width, 16 * width, 32 * width)


# ---------------------------------------------------------------------------------------------------------------- input and sizes
def scaled_input(img8) -> torch.Tensor:
    """[1][3][h][w] float32: step 1 of an HWC uint8 image."""
    x = torch.from_numpy(np.asarray(img8, np.float32) / np.float32(255.0))
    x = (x - torch.tensor(MEAN, dtype=torch.float32)) / torch.tensor(STD, dtype=torch.float32)
    assert x.dtype == torch.float32
    return x.permute(2, 0, 1)[None].contiguous()


def input_table() -> np.ndarray:
    """[3][256] float32: step 1 of every byte of every channel, by torch's float32 roundings."""
    v = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(3, axis=2)
    return scaled_input(v)[0, :, :, 0].numpy().copy()


def down2(s: int) -> int:
    return (s - 1) // 2 + 1


def level_sizes(h: int, w: int):
    """[(H, W)] of features 0 .. 4."""
    out = [(down2(h), down2(w))]
    H, W = down2(out[0][0]), down2(out[0][1])
    for s in STRIDES:
        if s == 2:
            H, W = down2(H), down2(W)
        out.append((H, W))
    return out


def token_sizes(h: int, w: int, variant=None):
    """[(H, W)] of the token grids of levels 0 .. 4: step 3's pooling condition."""
    sizes = level_sizes(h, w)
    th, tw = sizes[4]
    out = []
    for H, W in sizes:
        pooled = (H > th or W > tw) if variant == "pool_or" else (H > th and W > tw)
        out.append((th, tw) if pooled else (H, W))
    return out


def scorable(h: int, w: int) -> bool:
    return h >= MIN_EDGE and w >= MIN_EDGE


# ---------------------------------------------------------------------------------------------------------------- the model
def fold_bn(sd, bn: str):
    """(scale, shift) float32 of a frozen BatchNorm, folded in float64 and rounded once."""
    scale = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + BN_EPS)
    shift = sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * scale
    return scale.float(), shift.float()


def bicubic_axis(n_in: int, n_out: int, A: float = BICUBIC_A):
    """(taps [n_out][4] int64, weights [n_out][4] float64) of torch's bicubic along one axis: align_corners=False, clamped taps."""
    src = (n_in / n_out) * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5
    f = torch.floor(src)
    t = src - f
    c = torch.stack([((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                     ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1, ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A], dim=1)
    taps = (f.long()[:, None] + torch.arange(-1, 3)[None]).clamp(0, n_in - 1)
    return taps, c


def position_table(h_emb, w_emb, H: int, W: int, variant=None) -> torch.Tensor:
    """[D][H][W] float32: step 4, in float64 and rounded once. It depends on the size and the two embeddings alone."""
    hh = h_emb.double().expand(-1, -1, EMB_SIZE, EMB_SIZE)
    ww = w_emb.double().expand(-1, -1, EMB_SIZE, EMB_SIZE)
    src = torch.cat([ww, hh] if variant == "pos_halves_swapped" else [hh, ww], dim=1)[0]     # [D][32][32]
    ty, cy = bicubic_axis(EMB_SIZE, H, -0.5 if variant == "bicubic_a05" else BICUBIC_A)
    tx, cx = bicubic_axis(EMB_SIZE, W, -0.5 if variant == "bicubic_a05" else BICUBIC_A)
    g = src[:, :, tx] * cx                                                                   # [D][32][W][4]
    rows = ((g[..., 0] + g[..., 1]) + g[..., 2]) + g[..., 3]                                 # [D][32][W]
    g = rows[:, ty, :] * cy[None, :, :, None]                                                # [D][H][4][W]
    return (((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]) + g[:, :, 3]).float()


def adaptive_pool(x: torch.Tensor, th: int, tw: int, floor_end: bool = False) -> torch.Tensor:
    """adaptive_avg_pool2d of [1][C][H][W] written out: bin i covers floor(i H / th) .. ceil((i + 1) H / th) - 1; the sum runs over the bin's
    rows, inside a row over its columns, and is divided by the count."""
    H, W = x.shape[2:]
    out = x.new_zeros((x.shape[0], x.shape[1], th, tw))
    for i in range(th):
        y0, y1 = (i * H) // th, ((i + 1) * H) // th if floor_end else -((-(i + 1) * H) // th)
        for j in range(tw):
            x0, x1 = (j * W) // tw, ((j + 1) * W) // tw if floor_end else -((-(j + 1) * W) // tw)
            out[:, :, i, j] = x[:, :, y0:y1, x0:x1].sum(dim=(2, 3)) / ((y1 - y0) * (x1 - x0))
    return out


def score_image(img8, model, dtype=torch.float32, variant=None):
    """(score as a float, feat [D], the token mean of each level after its encoder layer [5][D]) of one HWC uint8 image, arrays in dtype."""
    img8 = np.asarray(img8)
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise TopiqError(f"an HWC uint8 RGB array is needed, got {img8.shape} {img8.dtype}")
    if not scorable(*img8.shape[:2]):
        raise TopiqError(f"TOPIQ needs at least {MIN_EDGE} x {MIN_EDGE} pixels; the image is {img8.shape[0]} x {img8.shape[1]}")
    dt = dtype
    sd, cfg = model["sd"], model["cfg"]
    D, heads = cfg["dim"], cfg["heads"]
    hd = D // heads
    approx = "tanh" if variant == "gelu_tanh" else "none"

    def t(key):
        return sd[key].to(dt)

    def conv(x, name, stride=1, pad=0, bias=False):
        return F.conv2d(x, t(name + ".weight"), t(name + ".bias") if bias else None, stride, pad)

    def bn(x, name):
        scale, shift = model["bn"][name]
        return x * scale.to(dt)[None, :, None, None] + shift.to(dt)[None, :, None, None]

    def ln(x, name):
        return F.layer_norm(x, (D,), t(name + ".weight"), t(name + ".bias"), LN_EPS)

    def mha(q_in, kv_in, p):
        Wi, bi = t(p + "attn.in_proj_weight"), t(p + "attn.in_proj_bias")
        Tq, Tk = q_in.shape[0], kv_in.shape[0]
        q = F.linear(q_in, Wi[:D], bi[:D]) * hd ** -0.5
        k = F.linear(kv_in, Wi[D:2 * D], bi[D:2 * D])
        v = F.linear(kv_in, Wi[2 * D:], bi[2 * D:])
        q, k, v = q.view(Tq, heads, hd).transpose(0, 1), k.view(Tk, heads, hd).transpose(0, 1), v.view(Tk, heads, hd).transpose(0, 1)
        o = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).transpose(0, 1).reshape(Tq, D)
        return F.linear(o, t(p + "attn.out_proj.weight"), t(p + "attn.out_proj.bias"))

    def ffn(x, p):
        return F.linear(F.gelu(F.linear(x, t(p + "linear1.weight"), t(p + "linear1.bias")), approximate=approx), t(p + "linear2.weight"), t(p + "linear2.bias"))

    def encoder_layer(x, p):
        if variant == "post_norm":
            x = ln(x + mha(x, x, p), p + "norm1")
            return ln(x + ffn(x, p), p + "norm2")
        y = ln(x, p + "norm1")
        x = x + mha(y, y, p)
        return x + ffn(ln(x, p + "norm2"), p)

    def decoder_layer(q, mem, p):
        """RECALLED FROM PYIQA (TransformerDecoderLayer of cfanet_arch, normalize_before), unpinned: no self-attention."""
        if variant == "post_norm":
            q = ln(q + mha(q, mem, p), p + "norm1")
            return ln(q + ffn(q, p), p + "norm3")
        m = mem if variant == "memory_not_normed" else ln(mem, p + "norm2")
        q = q + mha(ln(q, p + "norm1"), m, p)
        return q + ffn(ln(q, p + "norm3"), p)

    with torch.no_grad():
        x = scaled_input(img8).to(dt)
        feats = []
        x = F.relu(bn(conv(x, "trunk.conv1", 2, 3), "trunk.bn1"))
        feats.append(x)
        x = F.max_pool2d(x, 3, 2, 1)
        for l, depth in enumerate(cfg["depths"]):
            for b in range(depth):
                p = f"trunk.layer{l + 1}.{b}."
                s = STRIDES[l] if b == 0 else 1
                s1, s2 = (s, 1) if variant == "stride_on_conv1" else (1, s)
                y = F.relu(bn(conv(x, p + "conv1", s1), p + "bn1"))
                y = F.relu(bn(conv(y, p + "conv2", s2, 1), p + "bn2"))
                y = bn(conv(y, p + "conv3"), p + "bn3")
                idn = bn(conv(x, p + "downsample.0", s), p + "downsample.1") if b == 0 else x
                x = F.relu(y + idn)
            feats.append(x)

        th, tw = feats[4].shape[2:]
        tokens, means = [], []
        for i, f in enumerate(feats):
            g = f"gate.{i}."
            x1, x2 = conv(f, g + "split", bias=True).chunk(2, dim=1)
            if variant == "chunk_swapped":
                x1, x2 = x2, x1
            wgt = F.gelu(conv(x2, g + "conv1", bias=True), approximate=approx)
            wgt = F.gelu(conv(wgt, g + "conv2", 1, 1, bias=True), approximate=approx)
            wgt = torch.sigmoid(conv(wgt, g + "conv3", 1, 1, bias=True))
            m = F.gelu(x1, approximate=approx) * wgt
            H, W = m.shape[2:]
            if (H > th or W > tw) if variant == "pool_or" else (H > th and W > tw):
                m = adaptive_pool(m, th, tw, variant == "pool_floor_end")
            m = F.gelu(conv(m, f"reduce.{i}", bias=True), approximate=approx)
            m = m + position_table(sd["h_emb"], sd["w_emb"], m.shape[2], m.shape[3], variant).to(dt)[None]
            tok = encoder_layer(m[0].flatten(1).transpose(0, 1), f"sa.{i}.")
            tokens.append(tok)
            means.append(tok.mean(dim=0))

        query = tokens[0] if variant == "fine_to_coarse" else tokens[4]
        for k in range(4):
            mem = tokens[k + 1] if variant == "fine_to_coarse" else tokens[3 - k]
            query = decoder_layer(mem, query, f"ca.{k}.") if variant == "query_memory_swapped" else decoder_layer(query, mem, f"ca.{k}.")
        if variant == "mean_before_pool":
            feat = encoder_layer(query.mean(dim=0, keepdim=True), "pool.")[0]
        else:
            feat = encoder_layer(query, "pool.").mean(dim=0)
        y = F.gelu(F.linear(ln(feat, "score.0"), t("score.1.weight"), t("score.1.bias")), approximate=approx)
        y = F.gelu(F.linear(ln(y, "score.3"), t("score.4.weight"), t("score.4.bias")), approximate=approx)
        score = F.linear(y, t("score.6.weight"), t("score.6.bias"))[0]
    return float(score.double()), feat.numpy(), torch.stack(means).numpy()


def topiq(img8, model, dtype=torch.float32, variant=None) -> float:
    return score_image(img8, model, dtype, variant)[0]


# ---------------------------------------------------------------------------------------------------------------- loading
def config_of(sd, heads=None) -> dict:
    try:
        W = int(sd["trunk.conv1.weight"].shape[0])
        D = int(sd["reduce.4.weight"].shape[0])
        Fn = int(sd["sa.4.linear1.weight"].shape[0])
    except KeyError as e:
        raise TopiqError(f"no TOPIQ model: {e.args[0]} missing") from None
    depths = []
    for l in range(4):
        d = 0
        while f"trunk.layer{l + 1}.{d}.conv1.weight" in sd:
            d += 1
        depths.append(d)
    if min(depths) < 1:
        raise TopiqError(f"no TOPIQ model: trunk.layer{depths.index(0) + 1}.0.conv1.weight missing")
    heads = int(heads) if heads else DEFAULT_HEADS
    if D % 2 or heads < 1 or D % heads:
        raise TopiqError(f"the width {D} of the head is odd or no multiple of its {heads} heads")
    return dict(width=W, depths=tuple(depths), dim=D, heads=heads, ffn=Fn)


def _read(path):
    """({name: float32 tensor} in the project's names, heads or None) of an .npz in those names or of pyiqa's .pth (plain or under `params`)."""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            sd = {k: torch.from_numpy(np.asarray(z[k])).float() for k in z.files if k != "heads"}
            return sd, (int(z["heads"]) if "heads" in z.files else None)
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    for wrap in ("params", "state_dict"):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
    if not isinstance(sd, dict):
        raise TopiqError(f"{path}: no state dict")
    return from_pyiqa(sd, str(path)), None


def from_pyiqa(sd: dict, what: str = "the state dict") -> dict:
    """{project name: float32 tensor} of a state dict in pyiqa's names: every tensor of it is consumed or refused by name."""
    sd = {k: v.detach().float() for k, v in sd.items() if torch.is_tensor(v) and not k.endswith("num_batches_tracked")}
    for k in sd:
        if k.startswith("attn_blks.") and ".self_attn." in k:
            raise TopiqError(f"{what}: {k}: the coarse-to-fine layers of this model have no self-attention; a checkpoint with such tensors is another model")
    depths = []
    for l in range(4):
        d = 0
        while f"semantic_model.layer{l + 1}.{d}.conv1.weight" in sd:
            d += 1
        depths.append(d)
    back = {theirs: ours for ours, theirs in PYIQA_KEYS(depths).items()}
    for k in sd:
        if k not in back:
            raise TopiqError(f"{what}: {k} is no tensor of TOPIQ-NR")
    return {back[k]: v for k, v in sd.items()}


def to_pyiqa(model) -> dict:
    keys = PYIQA_KEYS(model["cfg"]["depths"])
    return {keys[k]: v.clone() for k, v in model["sd"].items()}


def load_model(path, heads=None) -> dict:
    """{sd: the tensors in the project's names (float32), bn: {bn name: (scale, shift)}, cfg}. path: an .npz, a .pth, or a dict in the project's
    names. A missing tensor, a surplus one or another shape raises TopiqError naming it."""
    if isinstance(path, dict):
        sd, h = {k: torch.as_tensor(v).detach().float() for k, v in path.items() if k != "heads"}, path.get("heads")
        h = int(h) if h is not None else None
    else:
        sd, h = _read(path)
    what = "the state dict" if isinstance(path, dict) else str(path)
    for k in sd:
        if k.startswith("ca.") and ".self_attn." in k:
            raise TopiqError(f"{what}: {k}: the coarse-to-fine layers of this model have no self-attention")
    try:
        cfg = config_of(sd, heads or h)
    except TopiqError as e:
        raise TopiqError(f"{what}: {e}") from None
    keys = model_keys(cfg)
    for k, shape in keys.items():
        if k not in sd:
            raise TopiqError(f"{what}: {k} missing")
        if tuple(sd[k].shape) != shape:
            raise TopiqError(f"{what}: {k} is {tuple(sd[k].shape)}, TOPIQ-NR of width {cfg['width']} and dim {cfg['dim']} has {shape}")
    for k in sd:
        if k not in keys:
            raise TopiqError(f"{what}: {k} is no tensor of TOPIQ-NR")
    sd = {k: sd[k].contiguous() for k in keys}
    return dict(sd=sd, cfg=cfg, bn={bn: fold_bn(sd, bn) for _, bn, *_ in trunk_convs(cfg["depths"])})


def save_npz(path, model) -> None:
    np.savez(path, heads=np.int64(model["cfg"]["heads"]), **{k: v.numpy() for k, v in model["sd"].items()})


# ---------------------------------------------------------------------------------------------------------------- the folder scorer
def evaluate(img_dir, model_path, ntest=None, backend="host", heads=None, log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    model = load_model(model_path, heads)
    ctx = tq = None
    if backend == "gpu":
        if _ROOT not in sys.path:
            sys.path.insert(0, _ROOT)
        from instarevive_amd import _lib as L, topiq as tq
        ctx = L.Context(0)
        tq.configure(ctx, model)
    total, scored, skipped, values = 0.0, 0, 0, {}
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            v = tq.score_arrays(ctx, img) if ctx is not None else topiq(img, model)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        values[f.name] = v
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"topiq_nr: {total / scored:.5f}")
    return (total / scored if scored else None), values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--topiq_model", required=True, help="the TOPIQ-NR weights: an .npz in this file's names, or pyiqa's .pth")
    ap.add_argument("--topiq_heads", type=int, default=None, help=f"the attention heads (a .pth does not record them; default {DEFAULT_HEADS})")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    try:
        evaluate(a.img_path, a.topiq_model, a.ntest, backend=a.backend, heads=a.topiq_heads)
    except TopiqError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    main()
