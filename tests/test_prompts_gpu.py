"""One prompt per image in a batched DiT call (ir_dit_set_prompts, AttnParams::kv_groups): the grouped cross-attention op against float64 softmax
attention and bit for bit against ir_op_attention on K / V expanded to every item; each image of a batch with per-image prompts bit-identical to the
same batch run with that image's prompt on every row (today's single-prompt path); process_stream with per-batch prompts; the command lines'
--caption_dir against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from instarevive_amd import _lib as L
from oracle import dit as odit
from oracle import glue as oglue
from oracle import swinir as oswin
from oracle import vae as ovae
from tests.golden._det import det_input
from tests.test_ops_gpu import P, close, dev_bf16, rb
from tests.test_models_gpu import (DIT_SMALL, PSNR_MIN, PSNR_STAGE1_MIN, SWIN_SMALL, VAE_SMALL, _oracle_process, _psnr_u8, _small_models,
                                   make_dit_control, make_swin, make_vae)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- op level
def _grouped_case(b, groups, heads, tq, tk, bias, seed):
    d = 72
    g = torch.Generator().manual_seed(seed)
    q = rb(torch.randn(b, tq, heads, d, generator=g))
    k = rb(torch.randn(groups, tk, heads, d, generator=g))
    v = rb(torch.randn(groups, tk, heads, d, generator=g))
    kb = None
    if bias == "quirk":      # the reference's 0 / 1 mask added to the logits
        kb = (torch.rand(groups, tk, generator=g) < 0.3).float()
    elif bias == "mask":
        kb = (torch.rand(groups, tk, generator=g) < 0.4).float() * -10000.0
        kb[:, 0] = 0
    elif bias == "spike":    # one late key 200 above everything in group 1 only: beyond the x72 kernel's fixed softmax reference
        kb = torch.zeros(groups, tk)
        kb[1, tk - 7] = 200.0
    return q, k, v, kb


def _run_grouped(ctx, q, k, v, kb, groups):
    b, tq, heads, d = q.shape
    tk = k.shape[1]
    o = torch.full((b, tq, heads, d), 0x7fc0, dtype=torch.int16, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_attention_kv_groups(ctx.h, ctx.stream(), P(dev_bf16(q)), P(dev_bf16(k)), P(dev_bf16(v)), P(o), b, heads, tq, tk, d,
                                                d ** -0.5, P(kb.cuda()) if kb is not None else None, groups, P(ws), ws.numel()), "attention_kv_groups")
    torch.cuda.synchronize()
    return L.from_bf16_bits(o).cpu()


def _run_expanded(ctx, q, k, v, kb, groups):
    b, tq, heads, d = q.shape
    tk = k.shape[1]
    idx = torch.arange(b) % groups
    ke, ve = k[idx].contiguous(), v[idx].contiguous()
    kbe = kb[idx].contiguous() if kb is not None else None
    o = torch.full((b, tq, heads, d), 0x7fc0, dtype=torch.int16, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_attention(ctx.h, ctx.stream(), P(dev_bf16(q)), P(dev_bf16(ke)), P(dev_bf16(ve)), P(o), b, heads, tq, tk, d, d ** -0.5,
                                      P(kbe.cuda()) if kbe is not None else None, P(ws), ws.numel()), "attention")
    torch.cuda.synchronize()
    return L.from_bf16_bits(o).cpu(), ke, ve, kbe


@pytest.mark.parametrize("route,b,groups,heads,tq,tk,bias", [
    ("x72", 4, 2, 16, 1024, 300, "quirk"), ("x72", 8, 4, 16, 512, 120, "mask"), ("x72", 4, 2, 16, 1024, 300, "spike"), ("x72", 4, 2, 16, 768, 128, "none"),
    ("generic", 4, 2, 4, 100, 40, "quirk"), ("generic", 8, 4, 2, 130, 77, "mask"), ("generic", 6, 3, 3, 64, 20, "none"),
    ("plain", 4, 2, 16, 1024, 300, "quirk"), ("plain", 8, 4, 16, 512, 120, "spike")])
def test_attention_kv_groups(ctx, route, b, groups, heads, tq, tk, bias):
    """x72 = flash_attn_x72_kernel (>= 64 items of 256 queries), generic = flash_attn_kernel<72, *> (small shapes), plain = ir_set_plain_kernels(1).
    Item i attends to K / V set i % groups; with a key bias (the DiT cross-attention form) the result is the bits of ir_op_attention given K / V
    expanded to one set per item, i.e. the same kernel on the same K / V."""
    q, k, v, kb = _grouped_case(b, groups, heads, tq, tk, bias, seed=b * 1000 + tq + tk)
    if route == "plain":
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "plain")
    try:
        got = _run_grouped(ctx, q, k, v, kb, groups)
        again = _run_grouped(ctx, q, k, v, kb, groups)
        exp, ke, ve, kbe = _run_expanded(ctx, q, k, v, kb, groups)
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "plain off")
    mask = kbe[:, None, None, :].double() if kbe is not None else None
    ref = F.scaled_dot_product_attention(q.double().transpose(1, 2), ke.double().transpose(1, 2), ve.double().transpose(1, 2), attn_mask=mask,
                                         scale=72 ** -0.5).transpose(1, 2).float()
    assert torch.equal(got, again), "grouped attention must be deterministic run to run"
    close(got, ref, 2 ** -6, 6e-3, f"grouped attention ({route})")
    if kb is not None:   # (without a bias ir_op_attention takes the self-attention kernel, which has no grouped form)
        assert torch.equal(got, exp), f"grouped attention ({route}) differs from the expanded K / V run"


def test_attention_kv_groups_refuses_uneven_groups(ctx):
    q, k, v, kb = _grouped_case(3, 2, 2, 64, 20, "quirk", seed=5)
    o = torch.empty(3, 64, 2, 72, dtype=torch.int16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.ir_op_attention_kv_groups(ctx.h, ctx.stream(), P(dev_bf16(q)), P(dev_bf16(k)), P(dev_bf16(v)), P(o), 3, 2, 64, 20, 72, 72 ** -0.5,
                                           P(kb.cuda()), 2, P(ws), ws.numel())
    assert rc != 0 and b"3 items" in ctx.lib.ir_last_error(ctx.h)


# ---------------------------------------------------------------------------------------------------------------- model level (reduced models)
def _three_prompts(cfg, ntok=20):
    """Three different prompts [3, T, C] and their 3-D masks [3, 1, T] (the CLI's additive form); prompt 1 has fewer real tokens."""
    ys = torch.cat([det_input(30 + i, (1, ntok, cfg["caption_channels"]), -1, 1) for i in range(3)])
    mask = torch.zeros(3, 1, ntok)
    for i, valid in enumerate((13, 6, 17)):
        mask[i, :, :valid] = 1
    return ys, mask


def _imgs(n, h, w, seed):
    return [(det_input(seed + i, (h, w, 3)) * 255).numpy().astype(np.uint8) for i in range(n)]


@pytest.mark.parametrize("tiled,fused,control,graph", [
    (False, True, False, False), (False, False, False, False), (True, True, False, False), (True, False, False, False),
    (False, True, True, False), (True, True, True, False), (False, True, False, True), (True, True, False, True)])
def test_per_image_prompts_match_single_prompt_batches(tiled, fused, control, graph):
    """A batch of 3 images with 3 prompts: image i is bit-identical to image i of the same batch run with prompt i on every row (the single-prompt
    path; same batch size, so every GEMM takes the same route and only the K / V slot differs), within 1 of a batch-1 run of image i alone, and
    (first configurations) within the oracle gates of the oracle run on the per-row prompts."""
    from instarevive_amd.pipeline import process
    cfg = dict(DIT_SMALL, num_layers=3) if control else DIT_SMALL
    (sw, sws), (vae, svae) = make_swin(SWIN_SMALL), make_vae(VAE_SMALL)
    if control:
        dit, sdit = make_dit_control(cfg, 2)
    else:
        from tests.test_models_gpu import make_dit
        dit, sdit = make_dit(cfg)
    ys, mask = _three_prompts(cfg)
    h, w = (128, 192) if tiled else (64, 128)
    imgs = _imgs(3, h, w, 500 + 10 * tiled)
    args = (1, "wavelet", False, tiled, 64, 32)
    kw = dict(preprocess_model=sw, vae=vae, fused=fused)
    got, got1 = process(dit, imgs, *args, y=ys.cuda(), y_mask=mask.cuda(), graph=graph, **kw)
    if graph:   # a replay with other prompt contents (same count and length): the recorded graph reads the new caches
        again, _ = process(dit, imgs, *args, y=ys.flip(0).cuda(), y_mask=mask.flip(0).cuda(), graph=True, **kw)
        flipped, _ = process(dit, imgs, *args, y=ys.flip(0).cuda(), y_mask=mask.flip(0).cuda(), **kw)
        assert all(np.array_equal(a, b) for a, b in zip(again, flipped))
        got, got1 = process(dit, imgs, *args, y=ys.cuda(), y_mask=mask.cuda(), graph=True, **kw)
    for i in range(3):
        yi, mi = ys[i:i + 1].expand(3, -1, -1).contiguous(), mask[i:i + 1].expand(3, -1, -1).contiguous()
        want, want1 = process(dit, imgs, *args, y=yi.cuda(), y_mask=mi.cuda(), **kw)
        assert np.array_equal(got[i], want[i]) and np.array_equal(got1[i], want1[i]), f"image {i}"
        alone, _ = process(dit, [imgs[i]], *args, y=ys[i:i + 1].cuda(), y_mask=mask[i:i + 1].cuda(), **kw)
        assert np.abs(got[i].astype(int) - alone[0].astype(int)).max() <= 1, f"image {i} vs batch 1"
    assert len({g.tobytes() for g in got}) == 3 and min(g.std() for g in got) > 1
    if not control and not graph:
        ref, ref1 = _oracle_process(imgs, sws, svae, sdit, ys, mask, color_fix_type="wavelet", tiled=tiled, tile_size=64, tile_stride=32)
        p, p1 = _psnr_u8(got, ref), _psnr_u8(got1, ref1)
        print(f"per-image prompts tiled={tiled} fused={fused}: PSNR vs oracle {p:.2f} dB (stage-1 {p1:.2f} dB)")
        assert p >= PSNR_MIN and p1 >= PSNR_STAGE1_MIN


def test_prompt_count_must_be_one_or_the_batch():
    from instarevive_amd.pipeline import process
    (sw, _), (vae, _), (dit, _) = _small_models()
    ys, mask = _three_prompts(DIT_SMALL)
    dit.set_prompt(ys.cuda(), mask.cuda())
    for fused in (True, False):
        with pytest.raises(RuntimeError, match="3 prompts are set for a batch of 2 images"):
            process(dit, _imgs(2, 64, 64, 600), 1, "wavelet", False, False, 64, 32, preprocess_model=sw, vae=vae, y=ys.cuda(), y_mask=mask.cuda(),
                    fused=fused)


def test_process_stream_per_batch_prompts():
    """process_stream over (images, y, y_mask) batches equals process() per batch bit for bit, with and without graph=True. Under graph=True the
    first two batches record (process_stream alternates two staging slots, so two call signatures), the third - other prompt contents, same count
    and length - replays the first one's recording, and the fourth, with one prompt (P 2 -> 1), records again."""
    from instarevive_amd.pipeline import process, process_stream
    (sw, _), (vae, _), (dit, _) = _small_models()
    ys, mask = _three_prompts(DIT_SMALL)
    batches = []
    for j in range(3):
        sel = [(j + 0) % 3, (j + 1) % 3]
        batches.append((_imgs(2, 64, 128, 700 + 10 * j), ys[sel].contiguous(), mask[sel].contiguous()))
    batches.append((_imgs(2, 64, 128, 740), ys[2:3].contiguous(), mask[2:3].contiguous()))
    args = ("wavelet", False, False, 64, 32)
    want = [process(dit, imgs, 1, *args, preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=m.cuda()) for imgs, y, m in batches]
    for graph in (False, True):
        dit.set_prompt(ys[:1].cuda(), mask[:1].cuda())   # one prompt set (ir_dit_set_prompt drops every recorded graph)
        r0 = dit.ctx.graph_records
        got = list(process_stream(dit, iter(batches), *args, preprocess_model=sw, vae=vae, graph=graph))
        assert len(got) == len(batches)
        for j, ((gp, g1), (wp, w1)) in enumerate(zip(got, want)):
            assert all(np.array_equal(a, b) for a, b in zip(gp, wp)) and all(np.array_equal(a, b) for a, b in zip(g1, w1)), (graph, j)
        assert dit.ctx.graph_records - r0 == (3 if graph else 0), (graph, dit.ctx.graph_records - r0)


# ---------------------------------------------------------------------------------------------------------------- full size
def test_full_size_two_prompts_1024(full_models):
    """The full DiT at 1024 x 1024 (x72 cross-attention in situ, 300-token prompts): each image of a batch of 2 with two prompts is bit-identical to
    the same batch run with its prompt on both rows."""
    from instarevive_amd.pipeline import process
    swin, vae, dit, sds, y, mask = full_models
    g = torch.Generator().manual_seed(77)
    y2 = torch.cat([y, torch.randn(y.shape, generator=g) * 0.1])
    m2 = torch.cat([mask, torch.zeros_like(mask)])
    m2[1, :, :60] = 1
    imgs = _imgs(2, 1024, 1024, 800)
    args = (1, "wavelet", False, False, 512, 448)
    got, _ = process(dit, imgs, *args, preprocess_model=swin, vae=vae, y=y2.cuda(), y_mask=m2.cuda(), return_stage1=False)
    for i in range(2):
        want, _ = process(dit, imgs, *args, preprocess_model=swin, vae=vae, y=y2[i:i + 1].expand(2, -1, -1).contiguous().cuda(),
                          y_mask=m2[i:i + 1].expand(2, -1, -1).contiguous().cuda(), return_stage1=False)
        assert np.array_equal(got[i], want[i]), f"image {i}"
        if i == 1:   # the prompts matter: image 0 under prompt 1 is another image
            assert not np.array_equal(got[0], want[0])


def test_set_prompts_does_not_wait_for_the_stream(full_models):
    """ir_dit_set_prompts is stream-ordered: with a 2048 x 2048 DiT step queued ahead of it, it returns while the stream is still busy."""
    swin, vae, dit, sds, y, mask = full_models
    y2 = torch.cat([y, y * 0.5]).cuda()
    b2 = torch.cat([mask, mask]).reshape(2, -1).cuda()
    dit.set_prompt(y2, torch.cat([mask, mask]).cuda())   # sizes the caches for two prompts (allocation is allowed to wait)
    lat = det_input(810, (1, 4, 256, 256), -2, 2).cuda()
    dit.set_prompt(full_models.y_cuda, full_models.mask_cuda)
    dit.step(lat, 400, 0.5, full_models.y_cuda, full_models.mask_cuda)
    torch.cuda.synchronize()
    ctx = dit.ctx
    dit.step(lat, 400, 0.5, full_models.y_cuda, full_models.mask_cuda)   # queued, not waited for
    stream = torch.cuda.current_stream()
    rc = ctx.lib.ir_dit_set_prompts(ctx.h, ctx.stream(), L.ptr(y2), L.ptr(b2), 2, y2.shape[1])
    busy = not stream.query()
    torch.cuda.synchronize()
    ctx.check(rc, "ir_dit_set_prompts")
    dit.invalidate_prompt()
    assert busy, "ir_dit_set_prompts waited for the work queued before it"


# ---------------------------------------------------------------------------------------------------------------- command lines
def _write_captions(d, names, ntok=20, dim=64):
    """Caption files in the reference's format for `names` (relative to d / "caps"); returns {name: (y [T, C], mask [T])}."""
    out = {}
    for i, nm in enumerate(names):
        y = det_input(900 + i, (1, ntok, dim), -1, 1)
        m = np.zeros((1, ntok), np.float32)
        m[:, :5 + 3 * i] = 1
        os.makedirs(os.path.dirname(d / "caps" / nm), exist_ok=True)
        if i % 2:
            np.savez(d / "caps" / nm, caption_feature=y.numpy())          # no attention_mask: all ones
            m[:] = 1
        else:
            np.savez(d / "caps" / nm, caption_feature=y.numpy(), attention_mask=m)
        out[nm] = (y.reshape(ntok, dim), torch.from_numpy(m).reshape(ntok))
    return out


def _oracle_one(x, sws, svae, sdit, y, m):
    return oglue.process([x], lambda t: oswin.swinir_forward(sws, t, SWIN_SMALL), lambda t: ovae.vae_encode_mean(svae, t, VAE_SMALL),
                         lambda lat, tt, yy, mm: odit.dit_forward(sdit, lat, tt, yy, mm, DIT_SMALL), lambda z: ovae.vae_decode(svae, z, VAE_SMALL),
                         oglue.alphas_cumprod_diffusers(), y.reshape(1, 20, 64), m.reshape(1, 1, 20))


def test_eval_batch_caption_dir_matches_oracle(tmp_path):
    from tests.test_cli_gpu import _write_artifacts
    from instarevive_amd.utils import center_crop_arr
    d = tmp_path
    sws, svae, sdit, y, mask = _write_artifacts(d)
    os.makedirs(d / "lq" / "sub", exist_ok=True)
    srcs = {"a.png": (70, 90), "b.jpg": (64, 64), "sub/c.png": (150, 130), "d.png": (64, 100), "e.png": (97, 71)}
    for i, (k, hw) in enumerate(srcs.items()):
        Image.fromarray((det_input(80 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "lq" / k, quality=95)
    caps = _write_captions(d, ["a.npz", "sub/c.npz", "e.npz", "d.npz"])   # b: no caption file (the --prompt_embeds prompt); sub/c: relative layout
    cmd = [sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "lq"), "--output",
           str(d / "res"), "--cond_output", str(d / "cond"), "--batch_size", "2", "--image_size", "64", "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"),
           "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"),
           "--caption_dir", str(d / "caps")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in srcs:
        name = os.path.splitext(k)[0] + ".png"
        got = np.array(Image.open(d / "res" / name).convert("RGB"))
        cy, cm = caps.get(os.path.splitext(k)[0] + ".npz", (y, mask))
        x = center_crop_arr(Image.open(d / "lq" / k).convert("RGB"), 64)
        ref, _ = _oracle_one(x, sws, svae, sdit, cy, cm)
        other, _ = _oracle_one(x, sws, svae, sdit, y, mask)
        p = _psnr_u8([got], ref)
        print(f"eval_batch --caption_dir {k}: PSNR vs oracle {p:.2f} dB (vs the fixed-prompt oracle {_psnr_u8([got], other):.2f} dB)")
        assert p >= 45.0


def test_inference_caption_dir_matches_oracle(tmp_path):
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    sws, svae, sdit, y, mask = _write_artifacts(d)
    os.makedirs(d / "in" / "sub", exist_ok=True)
    imgs = {f"{s}x{i}.png": (det_input(950 + i, (64, 64, 3)) * 255).numpy().astype(np.uint8) for i, s in enumerate(["", "sub/", "", "sub/"])}
    for k, v in imgs.items():
        Image.fromarray(v).save(d / "in" / k)
    caps = _write_captions(d, ["x0.npz", "sub/x1.npz", "x3.npz"])   # x2: the fixed prompt; x3: the flat layout of sub/x3.png
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
           str(d / "out"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
           "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--caption_dir", str(d / "caps")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k, v in imgs.items():
        got = np.array(Image.open(d / "out" / (os.path.splitext(k)[0] + "_0.png")).convert("RGB"))
        stem = os.path.splitext(os.path.basename(k))[0]
        cy, cm = caps.get(os.path.splitext(k)[0] + ".npz", caps.get(stem + ".npz", (y, mask)))
        lq = Image.fromarray(v)
        rs = oglue.auto_resize(lq, 512)
        ref, _ = _oracle_one(oglue.pad(np.array(rs), 64), sws, svae, sdit, cy, cm)
        want = np.array(Image.fromarray(ref[0][:rs.height, :rs.width]).resize(lq.size, Image.LANCZOS))
        p = _psnr_u8([got], [want])
        print(f"inference --caption_dir {k}: PSNR vs oracle {p:.2f} dB")
        assert p >= 47.0
