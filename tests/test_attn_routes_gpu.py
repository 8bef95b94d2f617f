"""Every attention route of the host layer (csrc/api.cpp: the d = 512 chain of the VAE mid block, the sharded part 0, the DiT self- and
cross-attention with their fp8, plain-kernel, KV-compression and prompt-slot forms, the UNet's transformer, the ir_op_attention* entry points) at
the smallest shape that still takes it, bit for bit against tests/golden/attn_routes.json.

That file was recorded by tests/golden/make_attn_routes.py with the library as it stood BEFORE the routes were gathered into one function each
(the parent commit's build, selected with INSTAREVIVE_HIP_LIB): per case the SHA-256 of the output bytes and the launches of every profiler row
(ctx.profile_begin() / ctx.profile_end_kernels()). The host layer chooses kernels, buffers and order, never arithmetic, so a route that is
written once must give the recorded digest and the recorded count of every row. The op entry points by-passed the profiler when the file was
recorded: their cases hold a digest and no counts ("launches": null).

One case has no recorded digest, by design: ir_op_attention_d512_fp8 with the gain-6 spike of test_ops_gpu.py::test_flash_attention_d512_fp8_spike
runs the product's chain (a flagged fp8 launch is recomputed by the bf16 d = 512 kernel), so its output must have exactly the bits of
ir_op_attention's d = 512 form on the same q / k / v, and the flag must be set.

At width 512 the route with the scores in HBM cannot be reached: a token count that is no multiple of 64 (6 x 6) is refused by transpose_v, whose
V^T rows are T + 64 keys long and must be whole 64-key tiles. That refusal is pinned as its code, and the route itself on a VAE of a quarter of
the width (mid block of 128 channels).

The whole file takes about 7 s on the MI355X, most of it the seeded model uploads it shares with test_vae_segment_gpu.py / test_dit_block_gpu.py.
"""
from functools import lru_cache
import hashlib
import json
import os

import pytest
import torch

from instarevive_amd import _lib as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_routes.json")
P = L.ptr


def digest(*tensors):
    """SHA-256 over the bytes of the tensors, in order."""
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def profiled(ctx, fn):
    """fn() under the profiler: (its result, {kernel row: launches})."""
    ctx.profile_begin()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        rows = ctx.profile_end_kernels()
    return out, {k: int(v["launches"]) for k, v in sorted(rows.items()) if v["launches"]}


def rb(t):
    return t.to(torch.bfloat16).float()


def dev_bf16(t):
    return t.to(torch.bfloat16).cuda().contiguous()


# ---------------------------------------------------------------- VAE mid block (attnblock)
@lru_cache(maxsize=None)
def vae_reduced():
    """A VAE of a quarter of the width (mid block of 128 channels): the only way into attnblock()'s route with the scores in HBM."""
    from tests.test_models_gpu import VAE_SMALL, make_vae
    return make_vae(VAE_SMALL)[0]


def vae_attn(req, n, h, w, wkind="base", fp8=False, plain=False, segment=None):
    """The decoder's mid.attn step alone (segment: a named segment of tests/support/vae_segment_ref.py instead) through ir_op_vae_segment."""
    from tests import test_vae_segment_gpu as VS
    from tests.support import vae_segment_ref as R
    m = vae_reduced() if wkind == "reduced" else VS.model(wkind)
    m._ready()
    ctx = m.ctx
    if segment:
        half, first, count = R.span(segment)
    else:
        half, first, count = 1, [s[0] for s in R.steps(1)].index("mid.attn"), 1
    width = 128 if wkind == "reduced" else R.in_channels(R.weights(wkind), half, first)
    x = R.make_input(n, width, h, w, seed=n * h * w + first, gain=R.input_scale(half, first), spike=wkind == "peaky")
    xd = x.cuda().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    extra = []
    try:
        if fp8:
            m.enable_fp8(True)
            ctx.check(ctx.lib.ir_set_fp8_mask(ctx.h, L.FP8_MASK_ATTENTION), "ir_set_fp8_mask")
        if plain:
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        if wkind == "peaky":   # the counting launch behind the chain, and the proof that the fp8 kernel's flag was raised
            ctx.check(ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 1), "ir_attn_fallback_count")
        (rc, y), rows = profiled(ctx, lambda: VS.launch(m, half, first, count, xd))
        extra.append(torch.tensor([rc], dtype=torch.int32))
        if rc != 0:   # a refusal is pinned as its code alone
            return digest(*extra), rows
        if wkind == "peaky":
            fb = ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 0)
            assert fb > 0, "the peaky case no longer raises the fp8 kernel's flag"
            extra.append(torch.tensor([fb], dtype=torch.int32))
        return digest(y, *extra), rows
    finally:
        if wkind == "peaky":
            ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), -1)
        ctx.lib.ir_set_plain_kernels(ctx.h, 0)
        if fp8:
            ctx.lib.ir_set_fp8_mask(ctx.h, L.FP8_MASK_DEFAULT)
            m.enable_fp8(False)
        ctx._ws = None


# ---------------------------------------------------------------- sharded part 0 (HipTileEngine.encode_part0)
def shard(req, r0, r1, force):
    import bench
    from instarevive_amd.pipeline import HipTileEngine
    fm = req.getfixturevalue("full_models")
    swin, vae, dit = fm[0], fm[1], fm[2]
    vae.enable_fp8(False)
    eng = HipTileEngine(dit, vae, swin, fm.y_cuda, fm.mask_cuda, "wavelet", False, 512, 448)
    img = [bench.synthetic_lq(1, 128, 128, 55)[0].numpy()]
    assert eng.can_shard_encode(img)

    def go():
        control, o, res = eng.encode_part0(img, r0, r1, force_fallback=force)
        flag = eng.encode_overflow()
        assert flag == int(force)
        return control, (o if force else o[r0:r1]), res, torch.tensor([flag], dtype=torch.int32)   # un-forced: only this rank's rows are written

    out, rows = profiled(eng.ctx, go)
    return digest(*out), rows


# ---------------------------------------------------------------- DiT block (dit_block)
def dit(req, n, gh, gw, prompts=1, kind="base", fp8=False, plain=False):
    from tests import test_dit_block_gpu as DB
    from tests.support import dit_block_ref as R
    W, m = DB.model(kind)
    ctx = m.ctx
    valid = (25, 61)[:prompts]
    y, bias = R.make_prompts(prompts, 300, valid, seed=prompts * 100 + sum(valid), form="cli" if prompts == 1 else "2d")
    DB.set_prompt(m, y, bias[:, None] if prompts == 1 else (bias == 0).float())
    x = R.make_tokens(n, gh * gw, seed=n * gh * gw)
    try:
        if fp8:   # the default mask leaves the DiT self-attention out
            ctx.check(ctx.lib.ir_set_fp8_mask(ctx.h, 1 << 0), "ir_set_fp8_mask")
            ctx.check(ctx.lib.ir_set_fp8(ctx.h, 1), "ir_set_fp8")
        if plain:
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        y_, rows = profiled(ctx, lambda: DB.block(m, x, n, gh, gw, "attention routes"))
        return digest(y_), rows
    finally:
        ctx.lib.ir_set_plain_kernels(ctx.h, 0)
        ctx.lib.ir_set_fp8(ctx.h, 0)
        ctx.lib.ir_set_fp8_mask(ctx.h, L.FP8_MASK_DEFAULT)
        m.invalidate_prompt()
        ctx._ws = None


# ---------------------------------------------------------------- UNet (uxf)
@lru_cache(maxsize=None)
def cldm_small():
    from tests.test_cldm_gpu import make_cldm
    return make_cldm()


def unet(req):
    from tests.golden._det import det_input
    from tests.test_cldm_gpu import CLDM_SMALL
    m, _ = cldm_small()
    zT = det_input(52, (1, 4, 16, 16), -2.0, 2.0)
    cond = {"c_concat": [torch.zeros(1, 3, 128, 128)], "c_crossattn": [det_input(71, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0)],
            "c_latent": [det_input(53, (1, 4, 16, 16), -2.0, 2.0)]}
    m.sample_log(cond, steps=1, zT=zT)   # (uploads, context caches)
    out, rows = profiled(m.ctx, lambda: m.sample_log(cond, steps=1, zT=zT))
    return digest(out), rows


# ---------------------------------------------------------------- op entry points
def qkv(b, heads, tq, tk, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (dev_bf16(torch.randn(b, tq, heads, d, generator=g)), dev_bf16(torch.randn(b, tk, heads, d, generator=g)),
            dev_bf16(torch.randn(b, tk, heads, d, generator=g)), torch.randn(b, tk, generator=g).cuda())


def op_attention(req, heads, d, tk=256, bias=False, groups=0):
    ctx = req.getfixturevalue("ctx")
    b, tq = (4 if groups else 1), 256
    q, k, v, kb = qkv(b, heads, tq, tk, d, seed=heads * 1000 + d + tk)
    o = torch.zeros(b, tq, heads, d, dtype=torch.int16, device="cuda")
    ws = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda")
    if groups:
        ctx.check(ctx.lib.ir_op_attention_kv_groups(ctx.h, ctx.stream(), P(q), P(k[:groups].contiguous()), P(v[:groups].contiguous()), P(o), b, heads, tq, tk, d,
                                                    d ** -0.5, P(kb[:groups].contiguous()) if bias else None, groups, P(ws), ws.numel()), "attention_kv_groups")
    else:
        ctx.check(ctx.lib.ir_op_attention(ctx.h, ctx.stream(), P(q), P(k), P(v), P(o), b, heads, tq, tk, d, d ** -0.5, P(kb) if bias else None,
                                          P(ws), ws.numel()), "attention")
    return digest(o), None


def op_attention_fp8(req):
    ctx = req.getfixturevalue("ctx")
    heads, t, d = 2, 256, 72
    q, k, v, _ = qkv(1, heads, t, t, d, seed=72008)
    o = torch.zeros(1, t, heads, d, dtype=torch.int16, device="cuda")
    ws = torch.zeros(16 << 20, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_attention_fp8(ctx.h, ctx.stream(), P(q), P(k), P(v), P(o), 1, heads, t, d ** -0.5, P(ws), ws.numel()), "attention_fp8")
    return digest(o), None


def d512_fp8(ctx, q, k, v, t):
    """ir_op_attention_d512_fp8 on [1][t][512] operands: (o, flag[0]). Workspace: tiles | flag | V^T | V^T tiles."""
    o = torch.zeros(1, t, 512, dtype=torch.int16, device="cuda")
    tiles = ((t // 64) * 66560 + 255) & ~255
    ws = torch.zeros(tiles + 256 + (t + 64) * 512 * 2 + ((t * 512 * 2 + 255) & ~255), dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_attention_d512_fp8(ctx.h, ctx.stream(), P(q), P(k), P(v), P(o), 1, t, 512 ** -0.5, P(ws), ws.numel()), "attention_d512_fp8")
    torch.cuda.synchronize()
    return o, int(ws[tiles:][:4].view(torch.int32)[0])


def op_attention_d512_fp8(req):
    ctx = req.getfixturevalue("ctx")
    q, k, v, _ = qkv(1, 1, 256, 256, 512, seed=512008)
    o, flag = d512_fp8(ctx, q, k, v, 256)
    assert flag == 0
    return digest(o), None


CASES = {
    "vae_8x8_n1": lambda r: vae_attn(r, 1, 8, 8),
    "vae_8x8_n2": lambda r: vae_attn(r, 2, 8, 8),
    "vae_8x8_plain": lambda r: vae_attn(r, 1, 8, 8, plain=True),
    "vae_6x6_refused": lambda r: vae_attn(r, 1, 6, 6),   # T = 36 at width 512: V^T has no padded row of T + 64 keys, transpose_v refuses (-2)
    "vae_reduced_8x8_generic": lambda r: vae_attn(r, 2, 8, 8, wkind="reduced"),   # width 128: scores and probabilities in HBM, image by image
    "vae_16x16_fp8": lambda r: vae_attn(r, 1, 16, 16, fp8=True),
    "vae_peaky_dec_mid": lambda r: vae_attn(r, 1, 64, 64, wkind="peaky", fp8=True, segment="dec_mid"),
    "shard_rows_0_128": lambda r: shard(r, 0, 128, False),
    "shard_rows_128_256": lambda r: shard(r, 128, 256, False),
    "shard_rows_0_128_forced": lambda r: shard(r, 0, 128, True),
    "shard_rows_128_256_forced": lambda r: shard(r, 128, 256, True),
    "dit_16x16": lambda r: dit(r, 1, 16, 16),
    "dit_16x16_fp8": lambda r: dit(r, 1, 16, 16, fp8=True),
    "dit_16x16_plain": lambda r: dit(r, 1, 16, 16, plain=True),
    "dit_8x8_n2": lambda r: dit(r, 2, 8, 8),
    "dit_12x20": lambda r: dit(r, 1, 12, 20),
    "dit_16x16_n2_prompts2": lambda r: dit(r, 2, 16, 16, prompts=2),
    "dit_16x16_qkn_kvc": lambda r: dit(r, 1, 16, 16, kind="qkn_kvc"),
    "dit_128x128": lambda r: dit(r, 1, 128, 128),
    "unet_step": unet,
    "op_d72_bias_tk300": lambda r: op_attention(r, 2, 72, tk=300, bias=True),
    "op_d72": lambda r: op_attention(r, 2, 72),
    "op_d64": lambda r: op_attention(r, 2, 64),
    "op_d32": lambda r: op_attention(r, 2, 32),
    "op_d512": lambda r: op_attention(r, 1, 512),
    "op_kv_groups": lambda r: op_attention(r, 2, 72, tk=300, bias=True, groups=2),
    "op_fp8": op_attention_fp8,
    "op_d512_fp8": op_attention_d512_fp8,
}


def record(name, req):
    """What the golden file holds for one case."""
    sha, rows = CASES[name](req)
    return {"sha256": sha, "launches": rows}


@lru_cache(maxsize=1)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_attn_route(case, request):
    want = golden()["cases"][case]
    got = record(case, request)
    print(f"ROUTE {case}: {got}")
    if want["launches"] is not None:
        assert got["launches"] == want["launches"], f"{case}: launches per profiler row differ from the recorded ones"
    assert got["sha256"] == want["sha256"], f"{case}: the output bytes differ from the recorded ones"


def test_attention_d512_fp8_flagged_launch_is_recomputed_by_the_bf16_kernel(ctx):
    """The gain-6 spike of test_flash_attention_d512_fp8_spike raises the fp8 kernel's flag; the entry point then runs the product's chain, whose
    rule is that a flagged fp8 launch is recomputed by the bf16 d = 512 kernel: the bits of ir_op_attention's d = 512 form on the same operands."""
    t, d, gain = 512, 512, 6.0
    g = torch.Generator().manual_seed(4)
    q = rb(torch.randn(1, t, d, generator=g))
    k = rb(torch.randn(1, t, d, generator=g))
    v = rb(torch.randn(1, t, d, generator=g))
    k[0, t - 6] = q[0, 7] * gain
    qd, kd, vd = dev_bf16(q), dev_bf16(rb(k)), dev_bf16(v)
    o8, flag = d512_fp8(ctx, qd, kd, vd, t)
    assert flag != 0, "the spike must raise the fp8 kernel's flag"
    o = torch.zeros(1, t, d, dtype=torch.int16, device="cuda")
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_attention(ctx.h, ctx.stream(), P(qd), P(kd), P(vd), P(o), 1, 1, t, t, d, d ** -0.5, None, P(ws), ws.numel()), "attention")
    torch.cuda.synchronize()
    assert torch.equal(o8, o), "behind the fp8 kernel's flag the result is not the bf16 d = 512 route's, bit for bit"
