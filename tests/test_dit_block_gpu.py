"""Op-level parity of one full-width PixArt DiT block (dit_block in csrc/api.cpp, through ir_op_dit_block) at the token counts the product runs,
against the float64 restatement in tests/support/dit_block_ref.py, evaluated on the GPU (attention chunked by query blocks).

The block runs layer 0 of a one-layer 16 x 72-head model (mlp 4608, caption 4096) uploaded by Transformer2DModel, with the prompt cache of
Transformer2DModel.set_prompt and the modulation tables of timestep 400, so the timestep gemv / t_block / modtab launches are under test too.
Gates act on the block's UPDATE (x_out - x_in): relative L2 <= 1e-2 and worst element <= 1e-2 of max |update| (the peaky case: 4e-2 / 8e-2, set
from its bf16 emulation with 2x margin - logits of std 37 magnify the rounding of q and k themselves). tests/test_dit_block_ref_cpu.py
shows that bf16 rounding at the HIP path's rounding points stays inside them with at least 2x margin and that every planted bug listed there
lands at least 1.5x outside. Each case also checks: a repeated launch gives the same bits; the same block under ir_set_plain_kernels(1) is inside
the gates and the fast route's rel-L2 is at most 1.15x the plain route's; the kernels the case is meant to reach did launch (profiler rows).
The 1024^2 batch case also checks that item 1 is bit-identical to that item run alone with its prompt alone.

Measured on the MI355X (fast route rel-L2 / worst; the plain route's rel-L2 is the same to three digits in every case, ratio 1.000):
    headline     2.44e-3 / 4.01e-3      ragged       2.64e-3 / 4.23e-3      peaky        1.78e-2 / 3.59e-2 (one fallback launch)
    batch_1024   2.73e-3 / 3.20e-3      small        3.60e-3 / 5.69e-3      qknorm_kvc   2.16e-3 / 2.75e-3
    tiles        3.12e-3 / 4.76e-3
"""
from functools import lru_cache

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import dit_block_ref as R

pytestmark = pytest.mark.gpu

FAST_OVER_PLAIN = 1.15
TIMESTEP = 400.0
K_GEMM_PP, K_SELF, K_CROSS, K_TRANSPOSE = ("linear/gemm_pp_kernel", "flash_attn/flash_attn_pp2_kernel (DiT self-attention)",
                                           "flash_attn/flash_attn_x72_kernel (DiT cross-attention)", "transpose/transpose_v*")

# id: items n, token grid gh x gw, prompts P, valid tokens per prompt, mask form, weights ('base', 'peaky', 'qkn_kvc'), expected profiler
# launches {kernel row: count} of the fast route (only the rows listed are checked). The transpose row counts vt_pad_init and transpose_v:
# at the headline only the former runs (the qkv epilogue writes V^T), the ragged grid has no V^T padding and transposes V.
CASES = {
    "headline": (1, 128, 128, 1, (25,), "cli", "base", {K_GEMM_PP: 6, K_SELF: 1, K_CROSS: 1, K_TRANSPOSE: 1}),
    "batch_1024": (2, 64, 64, 2, (25, 61), "2d", "base", {K_SELF: 1, K_CROSS: 1}),
    "tiles": (6, 32, 32, 1, (25,), "cli", "base", {K_SELF: 1, K_CROSS: 1}),
    "ragged": (1, 100, 68, 1, (25,), "cli", "base", {K_CROSS: 1, K_TRANSPOSE: 1}),
    "small": (1, 12, 20, 1, (25,), "cli", "base", {K_CROSS: 1}),
    "peaky": (1, 64, 64, 1, (25,), "cli", "peaky", {K_SELF: 1, K_CROSS: 1}),
    "qknorm_kvc": (1, 64, 64, 1, (25,), "cli", "qkn_kvc", {K_CROSS: 1}),
}


@lru_cache(maxsize=None)
def model(kind):
    """(DitWeights, Transformer2DModel) of one weight set, uploaded once."""
    from instarevive_amd.models import Transformer2DModel
    W = R.DitWeights(q_gain=R.PEAKY_GAIN * R.Q_GAIN if kind == "peaky" else R.Q_GAIN, qk_norm=kind == "qkn_kvc", kv_compress=kind == "qkn_kvc")
    kvc = dict(sampling="conv", scale_factor=2, kv_compress_layer=[0]) if W.kvc else None
    m = Transformer2DModel(num_attention_heads=R.HEADS, attention_head_dim=R.HD, num_layers=1, sample_size=64, caption_channels=R.CAP,
                           cross_attention_dim=R.C, kv_compress_config=kvc, qk_norm=W.qk_norm)
    m.load_state_dict(W.sd, strict=True)
    return W, m.to("cuda")


def prompts(case):
    n, gh, gw, P, valid, form, kind, _ = CASES[case]
    y, bias = R.make_prompts(P, 300, valid, seed=P * 100 + sum(valid), form=form)
    mask = bias[:, None] if form == "cli" else (bias == 0).float()   # what set_prompt takes: the 3-D mask as is, or the 2-D mask it converts
    return y, bias, mask


@lru_cache(maxsize=1)
def reference(case):
    n, gh, gw, P, valid, form, kind, _ = CASES[case]
    W, _ = model(kind)
    y, bias, _ = prompts(case)
    x = R.make_tokens(n, gh * gw, seed=n * gh * gw)
    with torch.no_grad():
        xd = x.cuda()
        ref = R.block(W, xd, R.modulation(W, TIMESTEP, "cuda"), tuple(t.cuda() for t in R.prompt_kv(W, y)), bias.cuda(), n, gh, gw).cpu()
    torch.cuda.empty_cache()
    return x, ref


def set_prompt(m, y, mask):
    m._ready()
    m.invalidate_prompt()
    m.set_prompt(y.cuda(), mask.cuda())


def run(m, x, n, gh, gw, layer=0):
    """ir_op_dit_block on a device copy of x (fp32): returns the launch's return code and the device rows."""
    ctx = m.ctx
    xd = x.float().cuda().contiguous()
    ws = ctx.workspace(ctx.ws_bytes(L.STAGE_DIT, n, 2 * gh, 2 * gw))
    rc = ctx.lib.ir_op_dit_block(ctx.h, ctx.stream(), L.ptr(xd), layer, n, gh, gw, TIMESTEP, L.ptr(ws), ws.numel())
    return rc, xd


def block(m, x, n, gh, gw, what):
    rc, xd = run(m, x, n, gh, gw)
    m.ctx.check(rc, what)
    torch.cuda.synchronize()
    assert torch.isfinite(xd).all(), what
    return xd


def gate(what, got, ref, x, kind):
    g_l2, g_worst = R.GATES["peaky" if kind == "peaky" else "base"]
    l2, worst = R.update_error(got.cpu(), ref, x)
    print(f"GATE {what}: rel-L2 {l2:.2e}, worst {worst:.2e}")
    assert l2 <= g_l2 and worst <= g_worst, f"{what}: rel-L2 {l2:.3e} (<= {g_l2}), worst {worst:.3e} (<= {g_worst})"
    return l2


@pytest.mark.parametrize("case", list(CASES))
def test_dit_block(case):
    n, gh, gw, P, valid, form, kind, routes = CASES[case]
    W, m = model(kind)
    ctx = m.ctx
    y, bias, mask = prompts(case)
    set_prompt(m, y, mask)
    x, ref = reference(case)
    what = f"dit_block {case} (n {n}, {gh} x {gw} tokens, P {P})"
    # fast route, twice: the second launch under the profiler (which kernels ran) and, for the peaky case, the fallback counter
    a = block(m, x, n, gh, gw, what)
    ctx.profile_begin()
    if kind == "peaky":
        ctx.check(ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 1), "ir_attn_fallback_count")
    b = block(m, x, n, gh, gw, what + " again")
    if kind == "peaky":
        fb = ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 0)
        ctx.check(ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), -1), "ir_attn_fallback_count")
        print(f"{what}: {fb} attention launch(es) took the fallback")
        assert fb > 0, f"{what}: the scores never outgrew the fixed softmax reference - the case does not reach the fallback"
    rows = ctx.profile_end_kernels()
    print(f"{what}: launches " + ", ".join(f"{k} x{v['launches']}" for k, v in sorted(rows.items())))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: two launches differ"
    for k, cnt in routes.items():
        got = rows.get(k, {}).get("launches", 0)
        assert got == cnt, f"{what}: {k} launched {got} times, expected {cnt}"
    l2_fast = gate(what, a, ref, x, kind)
    # the same block on the plain (4-wave) kernels
    try:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        c = block(m, x, n, gh, gw, what + " plain")
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
    l2_plain = gate(what + " plain", c, ref, x, kind)
    print(f"RATIO {what}: fast / plain rel-L2 {l2_fast / l2_plain:.3f}")
    assert l2_fast <= FAST_OVER_PLAIN * l2_plain, f"{what}: fast route rel-L2 {l2_fast:.3e} against the plain route's {l2_plain:.3e}"
    if n > 1 and P > 1:   # item 1 alone, with its prompt alone
        T = gh * gw
        set_prompt(m, y[1:2], mask[1:2])
        solo = block(m, x[T:2 * T], 1, gh, gw, what + " item 1 alone")
        assert torch.equal(a[T:2 * T].view(torch.int32), solo.view(torch.int32)), f"{what}: item 1 of the batch differs from item 1 run alone"


def test_dit_block_refuses_bad_arguments():
    """-1 for a layer out of range, -10 for an empty or negative grid, -12 for a prompt count other than 1 or n, -11 without a DiT."""
    W, m = model("base")
    y, bias, mask = prompts("batch_1024")
    set_prompt(m, y, mask)   # two prompt slots
    x = torch.zeros(2 * 4 * 4, R.C)
    for layer in (1, -1):
        assert run(m, x, 2, 4, 4, layer=layer)[0] == -1
    for gh, gw in ((0, 4), (4, 0), (-4, 4), (4, -4)):
        assert run(m, x, 2, gh, gw)[0] == -10, (gh, gw)
    assert run(m, torch.zeros(3 * 16, R.C), 3, 4, 4)[0] == -12
    assert run(m, x[:16], 1, 4, 4)[0] == -12
    bare = L.Context(0)   # a context without a DiT
    assert bare.lib.ir_op_dit_block(bare.h, bare.stream(), None, 0, 1, 4, 4, TIMESTEP, None, 0) == -11
