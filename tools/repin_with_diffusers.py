#!/usr/bin/env python3
"""Close the "parity unpinned" items the first time a box has the third-party packages this image lacks. NOT runnable in the build
container (no diffusers / open_clip / pyiqa, no network); documented so that one command does it where they exist:

    pip install diffusers==0.30.0 open_clip_torch pyiqa          # whichever are available; every section is skipped when its package is not
    python tools/repin_with_diffusers.py [--dit DIR] [--vae DIR] [--clip_tokens]   # writes tests/golden/diffusers_pins.npz, prints a verdict per item

What is unpinned today and how each item is pinned here. All of it is BEHAVIOUR OF CODE, not of weights, so seeded
random-initialised models of reduced width pin it exactly as the 4 GB checkpoints would; --dit / --vae additionally load real folders
(diffusers `from_pretrained` layouts) and run the same comparison at full size.

 1. diffusers Transformer2DModel (norm_type="ada_norm_single"), a 3-D `encoder_attention_mask` is ADDED to the cross-attention logits, a 2-D
    one becomes (1 - m) * -10000 (test_scripts/inference.py:274-277 passes 3-D): outputs for mask = None / 2-D / 3-D -> oracle.dit.dit_forward.
 2. PatchEmbed regenerates the sin-cos table for a latent that is not sample_size x sample_size with base_size = sample_size // patch_size
    (and `interpolation_scale`): a non-native, non-square latent -> oracle.dit.dit_forward / sincos_pos_embed.
 3. AutoencoderKL state-dict key names (to_q / to_k / to_v / to_out.0 against the legacy query / key / value / proj_attn) and the
    encode().latent_dist.mode() / decode().sample contract: a random-initialised AutoencoderKL's state dict -> oracle.vae + weights.pack_vae's
    expected keys.
 4. open_clip's text tower blocks and tokenizer (FrozenOpenCLIPEmbedder, ldm/modules/encoders/modules.py:171-193): a reduced CLIP text tower ->
    oracle.clip_text; open_clip.tokenize on sample prompts -> instarevive_amd.clip_bpe (needs open_clip's vocabulary file, which ships inside the
    open_clip package).
 5. pyiqa's PSNR-Y / SSIM-Y (evaluate_img.py:30-33) -> tools/evaluate_pairs.py.
 7. the `lpips` package's LPIPS(net="alex") (utils/metrics.py:41-66, evaluate_img.py:32) -> tools/evaluate_pairs.py::LPIPS on the package's own weights.
 8. pyiqa's NIQE (evaluate_img.py's `create_metric('niqe')`; defaults test_y_channel=True, color_space='yiq', crop_border=0) -> tools/evaluate_niqe.py on
    pyiqa's own niqe_modelparameters.mat: an image without flat areas (where the order of additions cannot matter) to 1e-6 relative, and one with
    a saturated patch, where pyiqa's convolution order decides the signs of y - mu; the deviation there is reported, not gated.
 9. pyiqa's CLIP-IQA (evaluate_img.py's `create_metric('clipiqa')`: OpenAI CLIP RN50 at the image's own size, no positional embedding in the
    attention pool, five antonym prompt pairs) -> tools/evaluate_clipiqa.py on pyiqa's own RN50 weights and vocabulary (pass --clip_bpe, the
    folder of the BPE table): the ten text rows and the score of two images to 1e-5.
10. OpenCV's side of the degradation chain (dataset/codeformer.py:151-163, utils/degradation.py:744-747) -> tools/degrade_folder.py: cv2.filter2D
    with a 41 x 41 kernel (a DFT path: to 1e-5 absolute, rounding only), cv2.resize INTER_LINEAR on floats down and up (bit-equal) and
    cv2.imencode / imdecode of a float image at three qualities (byte-equal).
11. pyiqa's MUSIQ (evaluate_img.py's `create_metric('musiq')`, the koniq10k checkpoint) -> tools/evaluate_musiq.py on pyiqa's own weights, read
    through PYIQA_KEYS: the score of two images to 1e-4 (the score is roughly 0 - 100; pyiqa runs fp32). A mismatch points at one of the three
    recollections that file names: the key table, standardize() or resize().
12. pyiqa's MANIQA (evaluate_img.py's `create_metric('maniqa')`, the koniq checkpoint) -> tools/evaluate_maniqa.py on pyiqa's own weights, read
    through PYIQA_KEYS, at pyiqa's uniform crop grid: the score of two images to 1e-5 (the score is roughly 0 - 1; pyiqa runs fp32). A mismatch
    points at one of that file's recollections: the key table, uniform_origins(), DEFAULTS (scale, crops, taps), or a step docs/parity.md lists.
13. pyiqa's DISTS (`create_metric('dists')`, the column papers print next to LPIPS) -> tools/evaluate_pairs.py::DISTS on pyiqa's own weights (its
    network's state dict, in the DISTS module's names): the score of two pairs to 1e-5 (pyiqa runs fp32). A mismatch points at one of the
    points docs/parity.md lists: the input range, the L2 pool's window and padding, map 0, the variance, the constants, the weights' sum.
14. pytorch-fid's InceptionV3(output_blocks=[3]) and pyiqa's `fid` input -> tools/evaluate_fid.py::InceptionFID on pytorch-fid's own weights: the
    2048 features of two images to 1e-5 of their largest (both run fp32) with the `legacy` input, pyiqa's / clean-fid's resized input against
    resize_clean() bit for bit, and calculate_frechet_distance against frechet_distance() on 4096 random features to 1e-6 relative. A mismatch
    points at one of the points docs/parity.md lists: eps, count_include_pad, the max pool of Mixed_7c, the branch order, the resize.
15. pyiqa's IL-NIQE (the `create_metric('ilniqe')` that evaluate_img.py keeps commented out) -> tools/evaluate_ilniqe.py on pyiqa's own
    ILNIQE_templateModel.mat: the score of two images without flat areas to 1e-3 relative (pyiqa scales its input in fp32). A mismatch points
    at one of the choices docs/parity.md lists as unpinned: the fp32 input scaling, the padding of the derivative convolutions, the resize
    order, the plane order, the unbiased std of the Weibull start.
16. pyiqa's TOPIQ-NR (the `create_metric('topiq_nr')` that evaluate_img.py keeps commented out) -> tools/evaluate_topiq.py on pyiqa's own weights,
    read through PYIQA_KEYS: the score of two images to 1e-5 (the score is roughly 0 - 1; pyiqa runs fp32). A mismatch points at one of that
    file's recollections: the key table, decoder_layer() (no self-attention), DEFAULT_HEADS, or a step docs/parity.md lists.
 6. ftfy.fix_text (diffusion/model/t5.py:118-124) -> instarevive_amd.captions.fix_text (deterministic steps + the restricted mojibake repair).

The fixture holds inputs, state-dict checksums and the third party's outputs (data, not source); tests/test_oracle_golden.py picks
tests/golden/diffusers_pins.npz up when it exists (test_diffusers_pins) and compares the oracle against it on every later run, on any box."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "diffusers_pins.npz")


def seeded_(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in sorted(model.named_parameters()):
            p.copy_((torch.rand(p.shape, generator=g) - 0.5) * (0.2 if p.ndim == 1 else 2 * (3.0 / max(1, int(np.prod(p.shape[1:])))) ** 0.5))
    return model


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-30))


def pin_dit(out, real_dir=None):
    from diffusers import Transformer2DModel
    from oracle import dit as odit
    cfg = dict(num_layers=2, num_attention_heads=2, attention_head_dim=8, in_channels=4, out_channels=8, patch_size=2, sample_size=8,
               caption_channels=32, interpolation_scale=1.0)
    if real_dir:
        m = Transformer2DModel.from_pretrained(real_dir).eval()
        c = m.config
        cfg = dict(num_layers=c.num_layers, num_attention_heads=c.num_attention_heads, attention_head_dim=c.attention_head_dim, in_channels=c.in_channels,
                   out_channels=c.out_channels, patch_size=c.patch_size, sample_size=c.sample_size, caption_channels=c.caption_channels,
                   interpolation_scale=getattr(c, "interpolation_scale", None) or max(c.sample_size // 64, 1))
    else:
        m = seeded_(Transformer2DModel(num_attention_heads=2, attention_head_dim=8, in_channels=4, out_channels=8, num_layers=2, cross_attention_dim=16,
                                       norm_type="ada_norm_single", sample_size=8, patch_size=2, caption_channels=32, norm_elementwise_affine=False,
                                       norm_eps=1e-6, attention_bias=True, activation_fn="gelu-approximate", num_embeds_ada_norm=1000), 11).eval()
    sd = {k: v.detach().float() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    ok = True
    for name, (h, w) in (("native", (cfg["sample_size"],) * 2), ("nonnative", (cfg["sample_size"] + 4, cfg["sample_size"] * 2 + 4))):
        lat = torch.randn(2, 4, h, w, generator=g)
        y = torch.randn(2, 6, cfg["caption_channels"], generator=g) * 0.3
        m2 = torch.tensor([[1, 1, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0]], dtype=torch.float32)
        for mname, mask in (("none", None), ("2d", m2), ("3d", m2[:, None, :])):
            with torch.no_grad():
                ref = m(lat, encoder_hidden_states=y, timestep=torch.tensor([400, 400]), encoder_attention_mask=mask,
                        added_cond_kwargs={"resolution": None, "aspect_ratio": None}).sample
            got = odit.dit_forward(sd, lat, torch.tensor([400.0, 400.0]), y, mask, cfg)
            e = rel(got, ref)
            ok &= e <= 1e-4
            print(f"  [1/2] Transformer2DModel {name} latent {h}x{w}, mask {mname}: oracle vs diffusers rel. L2 {e:.2e}")
            tag = f"dit_{'real_' if real_dir else ''}{name}_{mname}"
            out[tag + "_lat"], out[tag + "_y"], out[tag + "_out"] = lat.numpy(), y.numpy(), ref.numpy()
            if mask is not None:
                out[tag + "_mask"] = mask.numpy()
    if not real_dir:
        out["dit_cfg"] = np.array([cfg[k] for k in ("num_layers", "num_attention_heads", "attention_head_dim", "patch_size", "sample_size", "caption_channels")])
        for k, v in sd.items():
            out["dit_sd/" + k] = v.numpy()
    return ok


def pin_vae(out, real_dir=None):
    from diffusers import AutoencoderKL
    from instarevive_amd import weights as W
    from oracle import vae as ovae
    cfg = dict(ch=32, ch_mult=(1, 2), num_res_blocks=1)
    if real_dir:
        m = AutoencoderKL.from_pretrained(real_dir).eval()
        cfg = None
    else:
        m = seeded_(AutoencoderKL(in_channels=3, out_channels=3, down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2,
                                  block_out_channels=(32, 64), layers_per_block=1, latent_channels=4, norm_num_groups=32, sample_size=32), 12).eval()
    sd = {k: v.detach().float() for k, v in m.state_dict().items()}
    keys = set(sd)
    want = set(W.vae_shapes(cfg) if cfg else W.vae_shapes(dict(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2)))
    legacy = {k.replace("to_q", "query").replace("to_k", "key").replace("to_v", "value").replace("to_out.0", "proj_attn") for k in want}
    names_ok = keys == want or keys == legacy
    print(f"  [3] AutoencoderKL state-dict keys: {'match' if names_ok else 'DIFFER'} ({len(keys)} keys; "
          f"{'current to_q/... form' if keys == want else 'legacy query/... form' if keys == legacy else sorted(keys ^ want)[:6]})")
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(6)) * 2 - 1
    with torch.no_grad():
        z_ref = m.encode(x).latent_dist.mode()
        d_ref = m.decode(z_ref).sample
    e1, e2 = rel(ovae.vae_encode_mean(sd, x, cfg), z_ref), rel(ovae.vae_decode(sd, z_ref, cfg), d_ref)
    print(f"  [3] AutoencoderKL encode().latent_dist.mode(): oracle rel. L2 {e1:.2e}; decode().sample: {e2:.2e}")
    tag = "vae_real" if real_dir else "vae"
    out[tag + "_x"], out[tag + "_z"], out[tag + "_dec"] = x.numpy(), z_ref.numpy(), d_ref.numpy()
    if not real_dir:
        out["vae_keys"] = np.array(sorted(keys))
        for k, v in sd.items():
            out["vae_sd/" + k] = v.numpy()
    return names_ok and e1 <= 1e-4 and e2 <= 1e-4


def pin_clip(out):
    import open_clip
    from instarevive_amd.clip_bpe import ClipBPETokenizer
    from oracle import clip_text as oclip
    texts = ["", "a photo of a cat", "High-quality restoration of an OLD photograph, 4k & sharp!", "naïve café — 42 dogs"]
    want = open_clip.tokenize(texts)
    folder = os.path.dirname(open_clip.tokenizer.default_bpe())
    got = ClipBPETokenizer.from_folder(folder)(texts)
    tok_ok = bool(torch.equal(got, want))
    print(f"  [4] open_clip.tokenize vs instarevive_amd.clip_bpe on {len(texts)} prompts: {'identical' if tok_ok else 'DIFFER'}")
    out["clip_tokens"], out["clip_texts"] = want.numpy(), np.array(texts)
    tower_ok = True
    try:
        model = open_clip.model.CLIP(embed_dim=32, vision_cfg=dict(image_size=32, layers=1, width=32, patch_size=16),
                                     text_cfg=dict(context_length=77, vocab_size=49408, width=64, heads=2, layers=3)).eval()
        seeded_(model, 13)
        sd = {k: v.detach().float() for k, v in model.state_dict().items() if not k.startswith("visual.")}
        x = model.token_embedding(want) + model.positional_embedding
        x = x.permute(1, 0, 2)
        for i, r in enumerate(model.transformer.resblocks):
            if i == len(model.transformer.resblocks) - 1:   # layer "penultimate" (modules.py:185-186)
                break
            x = r(x, attn_mask=model.attn_mask)
        ref = model.ln_final(x.permute(1, 0, 2))
        got = oclip.encode_with_transformer(sd, want, dict(width=64, heads=2, layers=3, context_length=77, mlp_ratio=4.0, layer="penultimate"))
        e = rel(got, ref)
        tower_ok = e <= 1e-4
        print(f"  [4] open_clip text tower (3 blocks, penultimate): oracle rel. L2 {e:.2e}")
        out["clip_tower_out"] = ref.detach().numpy()
        for k, v in sd.items():
            out["clip_sd/" + k] = v.numpy()
    except Exception as ex:  # open_clip's constructor surface moves between versions: report, keep the tokenizer pin
        print(f"  [4] open_clip text tower: could not build the reduced model on this version ({ex})")
    return tok_ok and tower_ok


def pin_iqa(out):
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_pairs", os.path.join(ROOT, "tools", "evaluate_pairs.py"))
    ep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ep)
    g = torch.Generator().manual_seed(8)
    a = torch.rand(1, 3, 96, 128, generator=g)
    b = (a + 0.05 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    a8, b8 = (a * 255).round() / 255, (b * 255).round() / 255
    p_ref = float(pyiqa.create_metric("psnr", test_y_channel=True, color_space="ycbcr", device="cpu")(a8, b8))
    s_ref = float(pyiqa.create_metric("ssim", test_y_channel=True, color_space="ycbcr", device="cpu")(a8, b8))
    an, bn = a8[0].permute(1, 2, 0).numpy(), b8[0].permute(1, 2, 0).numpy()
    p, s = ep.psnr_y(an, bn), ep.ssim_y(an, bn)
    print(f"  [5] pyiqa PSNR-Y {p_ref:.4f} vs evaluate_pairs {p:.4f}; SSIM-Y {s_ref:.5f} vs {s:.5f}")
    out["iqa_a"], out["iqa_b"], out["iqa_psnr"], out["iqa_ssim"] = an, bn, np.float64(p_ref), np.float64(s_ref)
    return abs(p - p_ref) <= 1e-3 and abs(s - s_ref) <= 1e-4


def pin_lpips(out):
    """LPIPS v0.1 / alex as tools/evaluate_pairs.py restates it against the `lpips` package itself (utils/metrics.py:41-66), on the package's own weights."""
    import importlib.util
    import lpips
    spec = importlib.util.spec_from_file_location("evaluate_pairs", os.path.join(ROOT, "tools", "evaluate_pairs.py"))
    ep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ep)
    ref = lpips.LPIPS(net="alex").eval()
    mine = ep.LPIPS(None, {k: v for k, v in ref.state_dict().items()})
    g = torch.Generator().manual_seed(9)
    a = torch.rand(2, 3, 128, 160, generator=g)
    b = (a + 0.1 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    with torch.no_grad():
        want = ref(a, b, normalize=True).reshape(-1)
    got = mine(a, b, normalize=True)
    print(f"  [7] lpips package {want.tolist()} vs evaluate_pairs {got.tolist()}")
    out["lpips_a"], out["lpips_b"], out["lpips_ref"] = a.numpy(), b.numpy(), want.numpy()
    return bool(torch.allclose(got, want, rtol=1e-4, atol=1e-6))


def pin_niqe(out):
    """pyiqa's `niqe` against tools/evaluate_niqe.py on pyiqa's own pristine parameters. The model fixes the order of additions of the 7 x 7 filter;
    pyiqa inherits its convolution's, so only the image without flat areas is gated."""
    import importlib.util
    import pyiqa
    from pyiqa.archs.niqe_arch import NIQE   # noqa: F401  (its default weight file is what load_params must read)
    spec = importlib.util.spec_from_file_location("evaluate_niqe", os.path.join(ROOT, "tools", "evaluate_niqe.py"))
    en = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(en)
    metric = pyiqa.create_metric("niqe", device="cpu")
    path = None
    for root, _, names in os.walk(os.path.expanduser(os.environ.get("PYIQA_CACHE", "~/.cache/pyiqa"))):
        path = os.path.join(root, "niqe_modelparameters.mat") if "niqe_modelparameters.mat" in names else path
    if path is None:
        raise ImportError("pyiqa has not downloaded niqe_modelparameters.mat")
    mu, cov = en.load_params(path)
    rng = np.random.default_rng(10)
    yy, xx = np.mgrid[0:288, 0:384].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    plain = np.clip(np.rint(base + rng.normal(0, 4.0, base.shape)), 0, 255).astype(np.uint8)
    flat = plain.copy()
    flat[20:120, 40:200] = 255
    ok = True
    for name, img in (("plain", plain), ("flat", flat)):
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = en.niqe(img, mu, cov)
        print(f"  [8] pyiqa NIQE ({name}) {ref:.6f} vs evaluate_niqe {got:.6f} (relative {abs(got - ref) / ref:.2e})")
        out[f"niqe_{name}"], out[f"niqe_{name}_ref"] = img, np.float64(ref)
        if name == "plain":
            ok = abs(got - ref) <= 1e-6 * ref
    return ok


def pin_ilniqe(out):
    """pyiqa's `ilniqe` against tools/evaluate_ilniqe.py on pyiqa's own template. The model takes MATLAB's side wherever the two may differ
    (docs/parity.md), so a mismatch here names a choice to revisit, not a bug of the device code, which is tested against the model."""
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_ilniqe", os.path.join(ROOT, "tools", "evaluate_ilniqe.py"))
    ei = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ei)
    metric = pyiqa.create_metric("ilniqe", device="cpu")
    path = None
    for root, _, names in os.walk(os.path.expanduser(os.environ.get("PYIQA_CACHE", "~/.cache/pyiqa"))):
        path = os.path.join(root, "ILNIQE_templateModel.mat") if "ILNIQE_templateModel.mat" in names else path
    if path is None:
        raise ImportError("pyiqa has not downloaded ILNIQE_templateModel.mat")
    par = ei.load_params(path)
    rng = np.random.default_rng(15)
    ok = True
    for name, (h, w) in (("small", (288, 384)), ("large", (600, 1100))):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
        img = np.clip(np.rint(base + rng.normal(0, 6.0, base.shape)), 1, 254).astype(np.uint8)
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = ei.ilniqe(img, par)
        print(f"  [15] pyiqa IL-NIQE ({name}) {ref:.6f} vs evaluate_ilniqe {got:.6f} (relative {abs(got - ref) / ref:.2e})")
        out[f"ilniqe_{name}"], out[f"ilniqe_{name}_ref"] = img, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-3 * ref
    return ok


def pin_clipiqa(out, bpe=None):
    """pyiqa's `clipiqa` against tools/evaluate_clipiqa.py on the RN50 weights pyiqa itself loads (its CLIP model's state dict)."""
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_clipiqa", os.path.join(ROOT, "tools", "evaluate_clipiqa.py"))
    ec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ec)
    if bpe is None:
        raise ImportError("--clip_bpe (the folder of CLIP's BPE table) is needed to tokenise the prompts")
    metric = pyiqa.create_metric("clipiqa", device="cpu")
    sd = {k: v for k, v in metric.net.clip_model[0].state_dict().items()}
    model = ec.load_model(sd, bpe)
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:224, 0:288].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("smooth", 2.0), ("noisy", 25.0)):
        img = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = ec.clipiqa(img, model)
        print(f"  [9] pyiqa CLIP-IQA ({name}) {ref:.6f} vs evaluate_clipiqa {got:.6f} (absolute {abs(got - ref):.2e})")
        out[f"clipiqa_{name}"], out[f"clipiqa_{name}_ref"] = img, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-5
    return ok


def pin_maniqa(out):
    """pyiqa's `maniqa` against tools/evaluate_maniqa.py on the koniq weights pyiqa itself loads (its network's state dict, the ViT under `vit.`)."""
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_maniqa", os.path.join(ROOT, "tools", "evaluate_maniqa.py"))
    em = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(em)
    metric = pyiqa.create_metric("maniqa", device="cpu")
    sd = {k: v.detach().float() for k, v in metric.net.state_dict().items()}
    keys = em.PYIQA_KEYS(dict(vit_layers=em.DEFAULTS["taps"][-1] + 1, swin_depth=2))
    missing = [theirs for theirs in keys.values() if theirs not in sd]
    if missing:
        print(f"  [12] PYIQA_KEYS names {len(missing)} tensors pyiqa's checkpoint does not have, e.g. {missing[:3]}; it has e.g. {sorted(sd)[:5]}")
        return False
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:   # through the .pth reader, as a user's file goes
        torch.save(sd, os.path.join(tmp, "maniqa.pth"))
        model = em.load_model(os.path.join(tmp, "maniqa.pth"))
    net = metric.net
    print(f"  [12] pyiqa: scale {getattr(net.swintransformer1, 'scale', None)}, test_sample {getattr(net, 'test_sample', None)}; evaluate_maniqa: scale "
          f"{model['cfg']['scale']}, crops {model['cfg']['crops']}, taps {model['cfg']['taps']}")
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:288, 0:352].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("smooth", 2.0), ("noisy", 25.0)):
        img = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = em.maniqa(img, model)   # the uniform grid: current pyiqa's uniform_crop
        print(f"  [12] pyiqa MANIQA ({name}) {ref:.6f} vs evaluate_maniqa {got:.6f} (absolute {abs(got - ref):.2e})")
        out[f"maniqa_{name}"], out[f"maniqa_{name}_ref"] = img, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-5
    return ok


def pin_topiq(out):
    """pyiqa's `topiq_nr` against tools/evaluate_topiq.py on the weights pyiqa itself loads (its network's state dict)."""
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_topiq", os.path.join(ROOT, "tools", "evaluate_topiq.py"))
    et = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(et)
    metric = pyiqa.create_metric("topiq_nr", device="cpu")
    net = metric.net
    sd = {k: v.detach().float() for k, v in net.state_dict().items()}
    heads = getattr(getattr(net, "attn_pool", None), "self_attn", None)
    heads = getattr(heads, "num_heads", None)
    import tempfile
    try:
        with tempfile.TemporaryDirectory() as tmp:   # through the .pth reader, as a user's file goes
            torch.save(sd, os.path.join(tmp, "topiq.pth"))
            model = et.load_model(os.path.join(tmp, "topiq.pth"), heads)
    except et.TopiqError as ex:
        print(f"  [16] evaluate_topiq refuses pyiqa's state dict: {ex}; it has e.g. {sorted(sd)[:5]}")
        return False
    print(f"  [16] pyiqa: heads {heads}; evaluate_topiq: {model['cfg']}")
    rng = np.random.default_rng(19)
    yy, xx = np.mgrid[0:288, 0:352].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("smooth", 2.0), ("noisy", 25.0)):
        img = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = et.topiq(img, model)
        print(f"  [16] pyiqa TOPIQ-NR ({name}) {ref:.6f} vs evaluate_topiq {got:.6f} (absolute {abs(got - ref):.2e})")
        out[f"topiq_{name}"], out[f"topiq_{name}_ref"] = img, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-5
    return ok


def pin_dists(out):
    """pyiqa's `dists` against tools/evaluate_pairs.py::DISTS on the weights pyiqa itself loads."""
    import pyiqa
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_pairs", os.path.join(ROOT, "tools", "evaluate_pairs.py"))
    ep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ep)
    metric = pyiqa.create_metric("dists", device="cpu")
    sd = {k: v.detach().float() for k, v in metric.net.state_dict().items()}
    try:
        net = ep.DISTS(sd)
    except (KeyError, ValueError) as ex:
        print(f"  [13] pyiqa's state dict does not load into evaluate_pairs.DISTS: {ex}; it has e.g. {sorted(sd)[:6]}")
        return False
    rng = np.random.default_rng(19)
    yy, xx = np.mgrid[0:200, 0:264].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("near", 3.0), ("far", 30.0)):
        a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
        b = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        ta, tb = (torch.from_numpy(x).permute(2, 0, 1)[None].float() / 255.0 for x in (a, b))
        ref, got = float(metric(ta, tb)), float(net(ta, tb)[0])
        print(f"  [13] pyiqa DISTS ({name}) {ref:.7f} vs evaluate_pairs.DISTS {got:.7f} (absolute {abs(got - ref):.2e})")
        out[f"dists_{name}_a"], out[f"dists_{name}_b"], out[f"dists_{name}_ref"] = a, b, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-5
    return ok


def pin_fid(out):
    """pytorch-fid's network, pyiqa's resize and pytorch-fid's distance against tools/evaluate_fid.py on the weights pytorch-fid itself loads."""
    import importlib.util
    from pytorch_fid.fid_score import calculate_frechet_distance
    from pytorch_fid.inception import InceptionV3
    spec = importlib.util.spec_from_file_location("evaluate_fid", os.path.join(ROOT, "tools", "evaluate_fid.py"))
    ef = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ef)
    theirs = InceptionV3([3], resize_input=True, normalize_input=True).eval()
    try:   # fid_inception_v3() is the torchvision-named network whose blocks InceptionV3 re-groups: its state dict has the names the loader reads
        from pytorch_fid.inception import fid_inception_v3
        net = ef.InceptionFID({k: v.detach().float() for k, v in fid_inception_v3().state_dict().items()}, "fp32")
    except (KeyError, ValueError) as ex:
        print(f"  [14] pytorch-fid's state dict does not load into evaluate_fid.InceptionFID: {ex}")
        return False
    rng = np.random.default_rng(23)
    yy, xx = np.mgrid[0:200, 0:264].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("smooth", 3.0), ("noisy", 30.0)):
        a = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        with torch.no_grad():
            ref = theirs(torch.from_numpy(a).permute(2, 0, 1)[None].float() / 255.0)[0][0, :, 0, 0].numpy().astype(np.float64)
        got = net.features_of_images([a], "legacy")[0]
        rel = float(np.abs(got - ref).max() / np.abs(ref).max())
        print(f"  [14] pytorch-fid features ({name}) vs evaluate_fid.InceptionFID, legacy input: {rel:.2e} of the largest")
        out[f"fid_{name}_img"], out[f"fid_{name}_ref"] = a, ref
        ok = ok and rel <= 1e-5
    try:
        from pyiqa.archs.fid_arch import clean_resize   # pyiqa's name for clean-fid's resize; absent in some versions
        r = np.asarray(clean_resize(a))
        same = np.array_equal(np.asarray(r, np.float32), ef.resize_clean(a))
        print(f"  [14] pyiqa's clean resize vs evaluate_fid.resize_clean: {'bit-equal' if same else 'DIFFERENT'}")
        ok = ok and same
    except ImportError as ex:
        print(f"  [14] pyiqa's clean resize not compared: {ex}")
    fa, fb = rng.normal(0, 1, (4096, 2048)), rng.normal(0.05, 1.1, (4096, 2048))
    (m1, s1), (m2, s2) = ef.statistics(fa), ef.statistics(fb)
    ref, got = float(calculate_frechet_distance(m1, s1, m2, s2)), ef.frechet_distance(m1, s1, m2, s2)
    print(f"  [14] pytorch-fid distance {ref:.6f} vs evaluate_fid.frechet_distance {got:.6f}")
    return ok and abs(got - ref) <= 1e-6 * abs(ref)


def pin_musiq(out):
    """pyiqa's `musiq` against tools/evaluate_musiq.py on the koniq10k weights pyiqa itself loads (its network's state dict)."""
    import importlib.util
    import pyiqa
    spec = importlib.util.spec_from_file_location("evaluate_musiq", os.path.join(ROOT, "tools", "evaluate_musiq.py"))
    em = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(em)
    metric = pyiqa.create_metric("musiq", device="cpu")
    sd = {k: v.detach().float() for k, v in metric.net.state_dict().items()}
    layers = 0
    while em.PYIQA_KEYS(layers + 1)[f"layers.{layers}.ln1.weight"] in sd:
        layers += 1
    keys = em.PYIQA_KEYS(layers)
    missing = [theirs for theirs in keys.values() if theirs not in sd]
    if missing:
        print(f"  [11] PYIQA_KEYS names {len(missing)} tensors pyiqa's checkpoint does not have, e.g. {missing[:3]}; it has e.g. {sorted(sd)[:5]}")
        return False
    model = em.load_model({ours: (sd[theirs].reshape(sd[theirs].shape[-2:]) if ours in ("position_emb", "scale_emb") else sd[theirs].reshape(-1)
                                  if ours == "cls_token" else sd[theirs]) for ours, theirs in keys.items()})
    rng = np.random.default_rng(13)
    yy, xx = np.mgrid[0:224, 0:288].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 23) * np.cos(yy / 31), 128 + 70 * np.sin((xx + yy) / 41), 128 + 90 * np.cos(xx / 17 - yy / 29)], -1)
    ok = True
    for name, sigma in (("smooth", 2.0), ("noisy", 25.0)):
        img = np.clip(np.rint(base + rng.normal(0, sigma, base.shape)), 0, 255).astype(np.uint8)
        ref = float(metric(torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255.0))
        got = em.musiq(img, model)
        print(f"  [11] pyiqa MUSIQ ({name}) {ref:.6f} vs evaluate_musiq {got:.6f} (absolute {abs(got - ref):.2e})")
        out[f"musiq_{name}"], out[f"musiq_{name}_ref"] = img, np.float64(ref)
        ok = ok and abs(got - ref) <= 1e-4
    return ok


def pin_degrade(out):
    """cv2 against the steps of tools/degrade_folder.py that restate it: the blur (steps 2), the two resizes (3, 6) and the JPEG round trip (5)."""
    import cv2
    import importlib.util
    from instarevive_amd.degrade import bivariate_gaussian
    spec = importlib.util.spec_from_file_location("degrade_folder", os.path.join(ROOT, "tools", "degrade_folder.py"))
    dm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dm)
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:150, 0:203].astype(np.float64)
    img = np.clip(128 + 90 * np.sin(xx / 9)[..., None] * np.cos(yy / 13)[..., None] * np.array([1, .7, -.8]) + rng.normal(0, 12, (150, 203, 3)), 0, 255).astype(np.uint8)
    x = dm.to_float(img)
    k = bivariate_gaussian(41, 3.1, 0.8, 0.7, False)
    ref, got = cv2.filter2D(x, -1, k), dm.blur(x, k)
    d_blur = float(np.abs(ref - got).max())
    print(f"  [10] cv2.filter2D vs blur: largest difference {d_blur:.2e}")
    ok = d_blur <= 1e-5
    for (oh, ow) in ((61, 88), (150, 203), (75, 101)):
        src = got if (oh, ow) != (150, 203) else dm.bilinear(got, 61, 88)
        same = np.array_equal(cv2.resize(src, (ow, oh), interpolation=cv2.INTER_LINEAR), dm.bilinear(src, oh, ow))
        print(f"  [10] cv2.resize INTER_LINEAR {src.shape[:2]} -> {(oh, ow)}: {'bit-equal' if same else 'DIFFERENT'}")
        ok = ok and same
    low = np.clip(dm.bilinear(got, 61, 88), 0, 1)
    for q in (10, 60, 100):
        _, enc = cv2.imencode(".jpg", low[..., ::-1] * 255., [int(cv2.IMWRITE_JPEG_QUALITY), q])   # BGR, as the reference holds it
        ref8 = cv2.imdecode(enc, 1)[..., ::-1]
        same = np.array_equal(ref8, dm.jpeg_step(low, q)[1])
        print(f"  [10] cv2.imencode / imdecode at quality {q}: {'byte-equal' if same else 'DIFFERENT'}")
        ok = ok and same
    out["degrade_img"], out["degrade_kernel"], out["degrade_blur_ref"] = img, k, ref
    return ok


def pin_ftfy(out):
    import ftfy
    from instarevive_amd.captions import fix_text
    samples = ["caf\u00c3\u00a9 au lait", "it\u00e2\u20ac\u2122s a dog\u00e2\u20ac\u00a6", "\u00c3\u00a2\u00e2\u201a\u00ac\u00e2\u201e\u00a2 twice",
               "na\u00efve caf\u00e9", "\ufb01ne \uff21\uff22\uff23 \u201cq\u201d", "plain ascii", "&lt;b&gt; &amp;amp; x", "line\r\nbreak\u2028here"]
    want = [ftfy.fix_text(t) for t in samples]
    got = [fix_text(t) for t in samples]
    bad = [(t, w, g) for t, w, g in zip(samples, want, got) if w != g]
    print(f"  [6] ftfy.fix_text vs captions.fix_text on {len(samples)} samples: {'identical' if not bad else bad}")
    out["ftfy_samples"], out["ftfy_fixed"] = np.array(samples), np.array(want)
    return not bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dit", default=None, help="folder of a diffusers Transformer2DModel (the converted PixArt / InstaRevive transformer): also compare at full size")
    ap.add_argument("--vae", default=None, help="folder of the diffusers AutoencoderKL (sd-vae-ft-ema): also compare at full size")
    ap.add_argument("--clip_bpe", default=None, help="folder of CLIP's BPE table (bpe_simple_vocab_16e6.txt.gz): needed by item 9")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    out, verdict = {}, {}
    for name, fn, args in (("diffusers DiT (items 1, 2)", pin_dit, (None,)), ("diffusers VAE (item 3)", pin_vae, (None,)),
                           ("open_clip (item 4)", pin_clip, ()), ("pyiqa (item 5)", pin_iqa, ()), ("ftfy (item 6)", pin_ftfy, ()), ("lpips (item 7)", pin_lpips, ()),
                           ("pyiqa NIQE (item 8)", pin_niqe, ()), ("pyiqa CLIP-IQA (item 9)", pin_clipiqa, (a.clip_bpe,)),
                           ("OpenCV degradation steps (item 10)", pin_degrade, ()), ("pyiqa MUSIQ (item 11)", pin_musiq, ()),
                           ("pyiqa MANIQA (item 12)", pin_maniqa, ()), ("pyiqa DISTS (item 13)", pin_dists, ()), ("pytorch-fid / pyiqa FID (item 14)", pin_fid, ()),
                           ("pyiqa IL-NIQE (item 15)", pin_ilniqe, ()), ("pyiqa TOPIQ-NR (item 16)", pin_topiq, ())):
        print(name)
        try:
            verdict[name] = fn(out, *args)
        except ImportError as ex:
            print(f"  skipped: {ex}")
    if a.dit:
        print("diffusers DiT at full size")
        verdict["DiT, real folder"] = pin_dit(out, a.dit)
    if a.vae:
        print("diffusers VAE at full size")
        verdict["VAE, real folder"] = pin_vae(out, a.vae)
    if out:
        np.savez_compressed(a.out, **out)
        print("wrote", a.out)
    for k, v in verdict.items():
        print(f"{'PINNED ' if v else 'MISMATCH'}  {k}")
    return 0 if verdict and all(verdict.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
