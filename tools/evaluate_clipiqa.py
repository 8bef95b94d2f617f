#!/usr/bin/env python3
"""CLIP-IQA of an output folder: the no-reference metric `clipiqa` of the reference's evaluate_img.py (`create_metric('clipiqa')`).

    python tools/evaluate_clipiqa.py -i results/ --clipiqa_model RN50.pt --clip_bpe <folder with the BPE table> [--ntest N] [--backend gpu]

The reference takes it from pyiqa, which is not in this image, and the reference tree holds no CLIP code of its own. So the definition is RESTATED
here as a plain torch model from the published implementations (pyiqa's `clipiqa` default over OpenAI CLIP RN50) - parity with pyiqa itself is
unpinned until a box that has it runs tools/repin_with_diffusers.py. The pretrained RN50.pt does not exist offline either: the user passes it.
This file is the model ir_clipiqa (csrc/clipiqa.hip) is tested against; it runs on the CPU in float32 or float64.

  1. input: RGB bytes v; x = (v / 255 - mean) / std in float32, each step rounded in that order, mean = (0.48145466, 0.4578275, 0.40821073),
     std = (0.26862954, 0.26130258, 0.27577711). No resize, no crop; padding is 0 in this normalised domain.
  2. image tower: OpenAI CLIP's ModifiedResNet(layers, width, heads = width * 32 // 64, output_dim). No convolution has a bias, every
     BatchNorm is in eval mode with eps 1e-5. Stem: conv3x3(3 -> w/2, stride 2, pad 1), conv3x3(w/2 -> w/2, pad 1), conv3x3(w/2 -> w, pad 1),
     each with BatchNorm and ReLU, then AvgPool2d(2). Four layers of bottleneck blocks with planes w, 2w, 4w, 8w, the first block of layers
     2 - 4 with stride 2. Block: conv1x1-BN-ReLU, conv3x3(pad 1)-BN-ReLU, AvgPool2d(stride) when the stride is 2, conv1x1(-> 4 planes)-BN;
     identity branch AvgPool2d(stride) (stride 2) - conv1x1 - BN, present when the stride is 2 or the channel counts differ;
     relu(out + identity). The average pools are floor mode: an odd trailing row or column is dropped.
  3. attention pool: tokens [mean over HW, the HW tokens], NO positional embedding (pyiqa's pos_embedding=False), multi-head attention with
     separate q_proj / k_proj / v_proj (with bias), the query scaled by head_dim^-0.5, c_proj to output_dim; only token 0's output is used.
  4. text: CLIP's encode_text of the ten prompts PROMPTS (token + positional embedding, causal residual blocks with QuickGELU, ln_final, the
     row at the end-of-text token, @ text_projection), tokenised by instarevive_amd/clip_bpe.py; rows L2-normalised.
  5. score: f = feat / |feat|, logits = exp(logit_scale) * text @ f, softmax over each (positive, negative) pair, the mean of the five first
     entries.
Files are listed as evaluate_pairs.py lists them (glob "*.[jpJP][pnPN]*[gG]", sorted)."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
PROMPTS = ("Good image", "bad image", "Sharp image", "blurry image", "sharp edges", "blurry edges", "High resolution image", "low resolution image",
           "Noise-free image", "noisy image")
BN_EPS = 1e-5
MIN_EDGE = 32   # below it the tower's last map is empty
# what a wrong implementation might do instead; the tests show that the gate tells each apart
VARIANTS = ("ceil_pool", "pos_embedding", "no_mean_token", "no_q_scale", "relu_before_add", "identity_no_pool", "stem_stride1", "softmax_all", "pad_byte0")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ClipIqaError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------- input
def scaled_input(img8) -> torch.Tensor:
    """[1][3][h][w] float32: step 1 of an HWC uint8 image."""
    x = torch.from_numpy(np.asarray(img8, np.float32) / np.float32(255.0)).permute(2, 0, 1)[None]
    x = (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    assert x.dtype == torch.float32
    return x


def scale_table() -> np.ndarray:
    """[3][256] float32: step 1 of every byte of every channel, by torch's float32 roundings."""
    v = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(3, axis=2)
    return scaled_input(v)[0, :, :, 0].numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- the model's shape
def config_of(sd) -> dict:
    """layers, width, heads, out_dim, read off a state dict with OpenAI's names (`visual.*`)."""
    try:
        width = int(sd["visual.conv3.weight"].shape[0])
        out_dim = int(sd["visual.attnpool.c_proj.weight"].shape[0])
    except KeyError as e:
        raise ClipIqaError(f"no CLIP ModifiedResNet image tower: {e.args[0]} missing") from None
    layers = []
    for l in range(1, 5):
        n = 0
        while f"visual.layer{l}.{n}.conv1.weight" in sd:
            n += 1
        if n == 0:
            raise ClipIqaError(f"no CLIP ModifiedResNet image tower: visual.layer{l}.0.conv1.weight missing")
        layers.append(n)
    return dict(layers=tuple(layers), width=width, heads=width * 32 // 64, out_dim=out_dim)


def visual_keys(cfg) -> dict:
    """{key: shape} of the image tower's tensors (BatchNorm's num_batches_tracked and the attention pool's positional embedding are not used)."""
    w = cfg["width"]
    out = {}

    def conv_bn(conv, bn, cin, cout, ks):
        out[f"visual.{conv}.weight"] = (cout, cin, ks, ks)
        for v in ("weight", "bias", "running_mean", "running_var"):
            out[f"visual.{bn}.{v}"] = (cout,)

    conv_bn("conv1", "bn1", 3, w // 2, 3)
    conv_bn("conv2", "bn2", w // 2, w // 2, 3)
    conv_bn("conv3", "bn3", w // 2, w, 3)
    inplanes = w
    for l, count in enumerate(cfg["layers"]):
        planes = w << l
        for i in range(count):
            p = f"layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            conv_bn(p + "conv1", p + "bn1", inplanes, planes, 1)
            conv_bn(p + "conv2", p + "bn2", planes, planes, 3)
            conv_bn(p + "conv3", p + "bn3", planes, planes * 4, 1)
            if stride == 2 or inplanes != planes * 4:
                conv_bn(p + "downsample.0", p + "downsample.1", inplanes, planes * 4, 1)
            inplanes = planes * 4
    c = w * 32
    for name, rows in (("q_proj", c), ("k_proj", c), ("v_proj", c), ("c_proj", cfg["out_dim"])):
        out[f"visual.attnpool.{name}.weight"] = (rows, c)
        out[f"visual.attnpool.{name}.bias"] = (rows,)
    return out


# ---------------------------------------------------------------------------------------------------------------- image tower
def image_features(x: torch.Tensor, sd, cfg, variant=None, operand=None) -> torch.Tensor:
    """Steps 2 and 3: [n][out_dim] of the scaled input [n][3][h][w], in x's dtype (float32 or float64). variant: None or one of VARIANTS.
    operand: None, or a function applied to both operands of every convolution (a measurement of what narrower operands would cost)."""
    dt = x.dtype

    def t(key):
        return sd["visual." + key].to(dt)

    def conv_bn(x, conv, bn, relu, stride=1, pad=None):
        w = t(conv + ".weight")
        if operand is not None:
            x, w = operand(x), operand(w)
        x = F.conv2d(x, w, None, stride, w.shape[-1] // 2 if pad is None else pad)
        x = F.batch_norm(x, t(bn + ".running_mean"), t(bn + ".running_var"), t(bn + ".weight"), t(bn + ".bias"), False, 0.0, BN_EPS)
        return F.relu(x) if relu else x

    def pool(x):
        return F.avg_pool2d(x, 2, ceil_mode=variant == "ceil_pool")

    if variant == "pad_byte0":   # the border is the byte 0 pushed through step 1 instead of 0 in the normalised domain
        zero = scaled_input(np.zeros((1, 1, 3), np.uint8)).to(dt).view(1, 3, 1, 1)
        x = conv_bn(F.pad(x - zero, (1, 1, 1, 1)) + zero, "conv1", "bn1", True, 1 if variant == "stem_stride1" else 2, pad=0)
    else:
        x = conv_bn(x, "conv1", "bn1", True, 1 if variant == "stem_stride1" else 2)
    x = conv_bn(x, "conv2", "bn2", True)
    x = conv_bn(x, "conv3", "bn3", True)
    x = pool(x)
    for l, count in enumerate(cfg["layers"]):
        for i in range(count):
            p = f"layer{l + 1}.{i}."
            stride = 2 if (i == 0 and l > 0) else 1
            out = conv_bn(x, p + "conv1", p + "bn1", True)
            out = conv_bn(out, p + "conv2", p + "bn2", True)
            if stride == 2:
                out = pool(out)
            out = conv_bn(out, p + "conv3", p + "bn3", variant == "relu_before_add")
            idn = x
            if f"visual.{p}downsample.0.weight" in sd:
                if stride == 2 and variant == "identity_no_pool":   # the plain ResNet's strided 1 x 1 in place of pool + 1 x 1
                    idn = conv_bn(x, p + "downsample.0", p + "downsample.1", False, 2)[:, :, :out.shape[2], :out.shape[3]]
                else:
                    idn = conv_bn(pool(x) if stride == 2 else x, p + "downsample.0", p + "downsample.1", False)
            x = F.relu(out + idn)
    n, c, h, w = x.shape
    if h < 1 or w < 1:
        raise ClipIqaError("the image is too small: the tower's last map is empty")
    heads = cfg["heads"]
    hd = c // heads
    tok = x.flatten(2).permute(0, 2, 1)                      # [n][HW][c]
    mean = tok.mean(dim=1, keepdim=True)
    tok = tok if variant == "no_mean_token" else torch.cat([mean, tok], dim=1)
    if variant == "pos_embedding":   # CLIP's own attention pool adds one (randn / sqrt(c) at initialisation)
        g = torch.Generator().manual_seed(77)
        pe = (torch.randn(tok.shape[1], c, generator=g, dtype=torch.float64) / c ** 0.5).to(dt)
        tok, mean = tok + pe, mean + pe[:1]
    q = F.linear(mean, t("attnpool.q_proj.weight"), t("attnpool.q_proj.bias"))
    if variant != "no_q_scale":
        q = q * hd ** -0.5
    k = F.linear(tok, t("attnpool.k_proj.weight"), t("attnpool.k_proj.bias"))
    v = F.linear(tok, t("attnpool.v_proj.weight"), t("attnpool.v_proj.bias"))
    q = q.view(n, 1, heads, hd).transpose(1, 2)
    k = k.view(n, -1, heads, hd).transpose(1, 2)
    v = v.view(n, -1, heads, hd).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v   # [n][heads][1][hd]
    a = a.transpose(1, 2).reshape(n, c)
    return F.linear(a, t("attnpool.c_proj.weight"), t("attnpool.c_proj.bias"))


def pair_probabilities(feat: torch.Tensor, text: torch.Tensor, logit_scale_exp: float, variant=None) -> torch.Tensor:
    """Step 5 without the mean: [n][pairs], the probability of each pair's first prompt."""
    f = feat / feat.norm(dim=-1, keepdim=True)
    logits = logit_scale_exp * f @ text.to(feat.dtype).t()
    if variant == "softmax_all":
        return torch.softmax(logits, dim=-1).view(feat.shape[0], -1, 2)[..., 0]
    return torch.softmax(logits.view(feat.shape[0], -1, 2), dim=-1)[..., 0]


def score_images(imgs8, model, dtype=torch.float32, variant=None, operand=None):
    """(scores [n] float64 array, features [n][out_dim] array in dtype) of HWC uint8 images of one size."""
    x = torch.cat([scaled_input(i) for i in imgs8]).to(dtype)
    with torch.no_grad():
        feat = image_features(x, model["sd"], model["cfg"], variant, operand)
        prob = pair_probabilities(feat, model["text"], model["logit_scale_exp"], variant)
    return prob.mean(dim=1).double().numpy(), feat.numpy()


def clipiqa(img8, model, dtype=torch.float32, variant=None) -> float:
    img8 = np.asarray(img8)
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise ClipIqaError(f"an HWC uint8 RGB array is needed, got {img8.shape} {img8.dtype}")
    if min(img8.shape[:2]) < MIN_EDGE:
        raise ClipIqaError(f"CLIP-IQA needs at least {MIN_EDGE} x {MIN_EDGE} pixels; the image is {img8.shape[0]} x {img8.shape[1]}")
    return float(score_images([img8], model, dtype, variant)[0][0])


# ---------------------------------------------------------------------------------------------------------------- text side
def encode_text(sd, tokens: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """Step 4 before the normalisation: CLIP's encode_text of token rows [n][L] (L at most the context length), [n][out_dim]."""
    def t(key):
        return sd[key].to(dtype)

    n, L = tokens.shape
    x = t("token_embedding.weight")[tokens] + t("positional_embedding")[:L]
    width = x.shape[-1]
    heads = max(width // 64, 1)
    hd = width // heads
    mask = torch.full((L, L), float("-inf"), dtype=dtype).triu(1)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (width,), t(p + "ln_1.weight"), t(p + "ln_1.bias"), 1e-5)
        q, k, v = F.linear(h, t(p + "attn.in_proj_weight"), t(p + "attn.in_proj_bias")).chunk(3, dim=-1)
        q, k, v = (z.view(n, L, heads, hd).transpose(1, 2) for z in (q, k, v))
        a = torch.softmax((q * hd ** -0.5) @ k.transpose(-1, -2) + mask, dim=-1) @ v
        x = x + F.linear(a.transpose(1, 2).reshape(n, L, width), t(p + "attn.out_proj.weight"), t(p + "attn.out_proj.bias"))
        h = F.layer_norm(x, (width,), t(p + "ln_2.weight"), t(p + "ln_2.bias"), 1e-5)
        h = F.linear(h, t(p + "mlp.c_fc.weight"), t(p + "mlp.c_fc.bias"))
        h = h * torch.sigmoid(1.702 * h)   # QuickGELU
        x = x + F.linear(h, t(p + "mlp.c_proj.weight"), t(p + "mlp.c_proj.bias"))
        i += 1
    if i == 0:
        raise ClipIqaError("no CLIP text tower: transformer.resblocks.0.ln_1.weight missing")
    x = F.layer_norm(x, (width,), t("ln_final.weight"), t("ln_final.bias"), 1e-5)
    return x[torch.arange(n), tokens.argmax(dim=-1)] @ t("text_projection")   # the end-of-text token has the largest id


def tokenizer_of(bpe):
    """instarevive_amd/clip_bpe.py's tokenizer from a folder holding the BPE table (or the table's file), or `bpe` itself when it is one already."""
    if callable(bpe):
        return bpe
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    from instarevive_amd.clip_bpe import ClipBPETokenizer
    folder = os.fspath(bpe)
    return ClipBPETokenizer.from_folder(os.path.dirname(folder) if os.path.isfile(folder) else folder)


def text_features(sd, bpe, prompts=PROMPTS) -> torch.Tensor:
    """[len(prompts)][out_dim] float32: the L2-normalised text rows, computed on the CPU in float32."""
    tok = tokenizer_of(bpe)
    tokens = tok(list(prompts), int(sd["positional_embedding"].shape[0]))
    with torch.no_grad():
        return normalize_rows(encode_text(sd, tokens))


def normalize_rows(x) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).float()
    return (x / x.norm(dim=-1, keepdim=True)).contiguous()


# ---------------------------------------------------------------------------------------------------------------- loading
def _read(path):
    """{name: float32 tensor} of a TorchScript archive, a pickled state dict or an .npz."""
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(np.asarray(z[k])).float() for k in z.files}
    try:
        sd = torch.jit.load(str(path), map_location="cpu").state_dict()
    except RuntimeError:   # not a TorchScript archive
        sd = torch.load(str(path), map_location="cpu", weights_only=True)
        if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
            sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ClipIqaError(f"{path}: neither a TorchScript archive nor a state dict")
    return {k: v.detach().float() for k, v in sd.items() if torch.is_tensor(v)}


def load_model(path, bpe=None) -> dict:
    """The model of a user's OpenAI RN50.pt (a TorchScript archive or a plain state dict; weights upcast to float32) or of an .npz holding the
    same names. {sd, cfg, text [2 pairs][out_dim] float32 unit rows, logit_scale_exp}. The text rows are computed on the CPU from the text tower
    with the BPE table under `bpe`, or - an .npz may carry them - read from `text`, in which case no vocabulary is needed. A missing tensor or
    another shape raises ClipIqaError naming it."""
    sd = _read(path) if not isinstance(path, dict) else {k: torch.as_tensor(v).detach().float() for k, v in path.items()}
    what = "the state dict" if isinstance(path, dict) else str(path)
    try:
        cfg = config_of(sd)
    except ClipIqaError as e:
        raise ClipIqaError(f"{what}: {e}") from None
    for k, shape in visual_keys(cfg).items():
        if k not in sd:
            raise ClipIqaError(f"{what}: {k} missing")
        if tuple(sd[k].shape) != shape:
            raise ClipIqaError(f"{what}: {k} is {tuple(sd[k].shape)}, CLIP's ModifiedResNet of width {cfg['width']} has {shape}")
    if "logit_scale" not in sd:
        raise ClipIqaError(f"{what}: logit_scale missing")
    if "text" in sd:
        text = normalize_rows(sd["text"])
    else:
        if bpe is None:
            raise ClipIqaError(f"{what}: the prompts have to be tokenised - pass the folder that holds CLIP's BPE table (bpe_simple_vocab_16e6.txt.gz, "
                               f"or vocab.json + merges.txt)")
        try:
            text = text_features(sd, bpe)
        except KeyError as e:
            raise ClipIqaError(f"{what}: {e.args[0]} missing (CLIP's text tower)") from None
    if text.ndim != 2 or text.shape[0] % 2 or text.shape[1] != cfg["out_dim"] or not bool(torch.isfinite(text).all()):
        raise ClipIqaError(f"{what}: the text rows are {tuple(text.shape)}; pairs of rows of {cfg['out_dim']} finite values are needed")
    return dict(sd={k: v for k, v in sd.items() if k.startswith("visual.")}, cfg=cfg, text=text, logit_scale_exp=float(torch.exp(sd["logit_scale"].reshape(()))))


# ---------------------------------------------------------------------------------------------------------------- the folder scorer
def evaluate(img_dir, model_path, bpe=None, ntest=None, backend="host", log=print):
    from PIL import Image
    files = sorted(Path(img_dir).glob("*.[jpJP][pnPN]*[gG]"))[:ntest]
    if not files:
        raise SystemExit(f"no images under {img_dir}")
    model = load_model(model_path, bpe)
    ctx = cq = None
    if backend == "gpu":
        if _ROOT not in sys.path:
            sys.path.insert(0, _ROOT)
        from instarevive_amd import _lib as L, clipiqa as cq
        ctx = L.Context(0)
        cq.configure(ctx, model)
    total, scored, skipped = 0.0, 0, 0
    for f in files:
        img = np.asarray(Image.open(f).convert("RGB"))
        try:
            v = cq.score_arrays(ctx, img) if ctx is not None else clipiqa(img, model)
        except ValueError as e:
            skipped += 1
            log(f"{f.name}: not scored ({e})")
            continue
        total += v
        scored += 1
    log(f"Find {len(files)} images in {img_dir}" + (f" ({skipped} not scored)" if skipped else ""))
    if scored:
        log(f"clipiqa: {total / scored:.5f}")
    return total / scored if scored else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--img_path", required=True)
    ap.add_argument("--clipiqa_model", required=True, help="OpenAI CLIP's RN50.pt (TorchScript archive or state dict), or an .npz with the same names")
    ap.add_argument("--clip_bpe", default=None, help="folder with CLIP's BPE table (bpe_simple_vocab_16e6.txt.gz, or vocab.json + merges.txt); not needed "
                    "when the .npz carries `text`")
    ap.add_argument("--ntest", type=int, default=None)
    ap.add_argument("--backend", choices=("host", "gpu"), default="host")
    a = ap.parse_args()
    try:
        evaluate(a.img_path, a.clipiqa_model, a.clip_bpe, a.ntest, backend=a.backend)
    except ClipIqaError as e:
        raise SystemExit(str(e))


if __name__ == "__main__":
    main()
