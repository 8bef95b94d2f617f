"""Op-level parity of the fused SwinIR block kernels (csrc/swin_fused.hip) through their C-ABI entries ir_op_swin_block, ir_op_swin_attn_proj and
ir_op_swin_mlp, against the fp32 restatement of one SwinTransformerBlock in tests/support/swin_block_ref.py (production weights.pack_swinir
layouts on bf16-rounded det_state_dict weights).

Gates act on the block's UPDATE (out - x_in), which the residual stream hides in `out`: relative L2 <= 1e-2 and worst element <= 1e-2 of
max |update|. tests/test_swin_block_ref_cpu.py shows that bf16 rounding at the kernels' rounding points stays inside them with more than 2x
margin (about 2.4e-3 / 2.7e-3), and that a transposed bias table, a LayerNorm over 192 channels, two heads' V swapped, an unmasked window
class, a reversed roll or one dropped fc2 bias channel lands at least 1.5x outside. Measured on the MI355X (rel-L2 / worst, every case and form):
    swin_block_kernel       2.17e-3 .. 2.41e-3 / 2.16e-3 .. 3.05e-3   (the unfused launch chain on the same inputs: the same values, RMS ratio 1.000)
    swin_attn_proj_kernel   1.90e-3 .. 1.96e-3 / 1.56e-3 .. 2.16e-3
    swin_mlp_kernel         2.30e-3 .. 2.42e-3 / 2.36e-3 .. 2.75e-3
Besides the gates, every case checks: in-place and out-of-place launches and a repeated launch are bit-identical, image 1 of a batched run
is bit-identical to a run of that image alone (every wave's arithmetic is private), padded channels are exactly 0, and each out2 form is
measured against the launch's own x_out (bf16 copy / next block's LayerNorm / next block's qkv rows)."""
import math
from functools import lru_cache

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import swin_block_ref as R

pytestmark = pytest.mark.gpu

GATE_L2, GATE_WORST = 1e-2, 1e-2
FORMS = ("copy", "ln1", "qkv")   # swin_block_kernel / swin_mlp_kernel <false, false>, <true, false>, <true, true>


def close(got, ref, rtol, atol, what=""):
    err = (got - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max abs err {err.max():.4g}, ref max {ref.abs().max():.4g}"


def same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@lru_cache(maxsize=None)
def weights(C, hid, bias_gain):
    w = R.BlockWeights(C, hid, bias_gain=bias_gain)
    w.dev = {k: v.cuda() for k, v in w.packed.items() if k.startswith("swin.l0.b")}
    return w


# id: B, H, W, shift, C, hidden units, peaky (bias table x 16, q x 4)
CASES = {
    "product_s0": (1, 64, 64, 0, 180, 360, False),      # the 512 px SwinIR input
    "product_s4": (1, 64, 64, 4, 180, 360, False),
    "batch_s0": (2, 24, 40, 0, 180, 360, False),        # 15 windows per image: a workgroup of four windows straddles the images, the last is ragged
    "batch_s4": (2, 24, 40, 4, 180, 360, False),
    "window_s0": (1, 8, 8, 0, 180, 360, False),         # one window: six of eight waves idle
    "window_s4": (1, 8, 8, 4, 180, 360, False),         # ... and only window class 3
    "row_s4": (1, 8, 40, 4, 180, 360, False),           # one window row
    "nopad_s4": (2, 24, 40, 4, 192, 512, False),        # head dim 32, hid_p at the 512 limit
    "ring32_s4": (1, 24, 40, 4, 180, 30, False),        # hid_p 32: a one-step weight ring
    "ring64_s0": (1, 24, 40, 0, 180, 64, False),
    "bench_b8_s4": (8, 64, 64, 4, 180, 360, False),     # bench.py's batch
    "peaky_s4": (1, 64, 64, 4, 180, 360, True),
}


@lru_cache(maxsize=None)
def reference(case):
    B, H, W_, shift, C, hid, peaky = CASES[case]
    w = weights(C, hid, 16.0 if peaky else 1.0)
    j = 1 if shift else 0   # block 1 of the RSTB is the shifted one (biasM); both have a next block with qkv_t
    x, qkv = R.make_inputs(w, j, B, H, W_, seed=B * H * W_ + shift, q_gain=4.0 if peaky else 1.0)
    return w, j, x, qkv, R.block(w, j, qkv, x, B, H, W_, shift)


def gate(what, got, ref, x):
    l2, worst = R.update_error(got, ref, x)
    print(f"GATE {what}: rel-L2 {l2:.2e}, worst {worst:.2e}")
    assert l2 <= GATE_L2 and worst <= GATE_WORST, f"{what}: rel-L2 {l2:.3e} (<= {GATE_L2}), worst {worst:.3e} (<= {GATE_WORST})"


def check_rows(w, got, what):
    assert torch.isfinite(got).all(), what
    if w.C < R.CP:
        assert got[:, w.C:].abs().max() == 0, f"{what}: padded residual channels are not 0"


def check_out2(w, j, form, xo, o2, what):
    """out2 against the launch's own x_out: the bf16 copy bit for bit, the next block's norm1 rows within bf16 rounding of the fp32 LayerNorm,
    its qkv rows within test_linear's tolerance (2e-4 sqrt(k), bf16-output rtol 2^-7) of bf16(LN(x_out)) Wqkv^T + b."""
    nb = w.p(j + 1)
    if form == "copy":
        assert torch.equal(o2, L.bf16_bits(xo)), f"{what}: out2 is not the RNE bf16 copy of x_out"
        return
    ln = R.layer_norm_rows(xo, w.sd[nb + "norm1.weight"], w.sd[nb + "norm1.bias"], w.C)
    got = L.from_bf16_bits(o2)
    if form == "ln1":
        if w.C < R.CP:
            assert got[:, w.C:].abs().max() == 0, f"{what}: out2 padding is not 0"
        close(got, ln, 2 ** -7, 2e-3, f"{what}: next norm1 rows")
        return
    assert got.shape[1] == R.LDQ
    if w.hd < 32:
        assert got.view(-1, 18, 32)[..., w.hd:].abs().max() == 0, f"{what}: qkv head columns {w.hd}..31 are not 0"
    close(got, R.qkv_rows(R.rb(ln), *w.qkv_dev(j + 1)), 2 ** -7, 2e-4 * math.sqrt(R.CP), f"{what}: next qkv rows")


def run_block(ctx, w, j, shift, B, H, W_, qkv, x_in, x_out, out2, form):
    D, d, n = w.dev, w.d(j), w.d(j + 1)
    nxt, tail = form in ("ln1", "qkv"), form == "qkv"
    p = L.ptr
    return ctx.lib.ir_op_swin_block(ctx.h, ctx.stream(), p(qkv), p(x_in), p(x_out), p(out2), p(D[d + "proj_t"]), p(D[d + "proj.b"]),
                                    p(D[d + ("biasM" if shift else "biasT")]), B, H, W_, shift, w.hd ** -0.5, p(D[d + "mlp_t"]), p(D[d + "mlp_v"]),
                                    w.C, w.hid_p, 1e-5, p(D[n + "n1.g"]) if nxt else None, p(D[n + "n1.b"]) if nxt else None,
                                    p(D[n + "qkv_t"]) if tail else None, p(D[n + "qkv.b"]) if tail else None, R.LDQ if tail else 0)


def out2_buf(T, form):   # filled with a finite non-zero pattern: a padding element the kernel does not write fails the zero checks
    return torch.full((T, R.LDQ if form == "qkv" else R.CP), 0x3f3f, dtype=torch.int16, device="cuda")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(CASES))
def test_swin_block(ctx, case, form):
    B, H, W_, shift, C, hid, _ = CASES[case]
    w, j, x, qkv, ref = reference(case)
    T, what = B * H * W_, f"swin_block {case} {form}"
    qkv_d, x_d = L.bf16_bits(qkv).cuda(), x.cuda()
    outs = []
    for _ in range(2):   # out of place, twice
        xo, o2 = torch.full((T, R.CP), float("nan"), device="cuda"), out2_buf(T, form)
        ctx.check(run_block(ctx, w, j, shift, B, H, W_, qkv_d, x_d, xo, o2, form), what)
        outs.append((xo, o2))
    # in place, as the model runs blocks 1..: x_in == x_out, and in the qkv form out2 is the qkv tensor the launch reads
    xi = x_d.clone()
    o2i = qkv_d.clone() if form == "qkv" else out2_buf(T, form)
    ctx.check(run_block(ctx, w, j, shift, B, H, W_, o2i if form == "qkv" else qkv_d, xi, xi, o2i, form), what + " in place")
    torch.cuda.synchronize()
    xo, o2 = outs[0]
    assert same_bits(xo, outs[1][0]) and torch.equal(o2, outs[1][1]), f"{what}: two launches differ"
    assert same_bits(xo, xi) and torch.equal(o2, o2i), f"{what}: in-place and out-of-place results differ"
    if B > 1:   # image 1 alone
        s = slice(H * W_, 2 * H * W_)
        q1, x1 = qkv_d[s].clone(), x_d[s].clone()
        xo1, o21 = torch.full((H * W_, R.CP), float("nan"), device="cuda"), out2_buf(H * W_, form)
        ctx.check(run_block(ctx, w, j, shift, 1, H, W_, q1, x1, xo1, o21, form), what + " image 1")
        torch.cuda.synchronize()
        assert same_bits(xo[s], xo1) and torch.equal(o2[s], o21), f"{what}: image 1 of the batch differs from image 1 alone"
    got = xo.cpu()
    check_rows(w, got, what)
    gate(what, got, ref["out"], x)
    check_out2(w, j, form, got, o2.cpu(), what)


@pytest.mark.parametrize("case", list(CASES))
def test_swin_block_against_the_unfused_chain(ctx, case):
    """The fused block's RMS error against the fp32 reference is at most 1.1x that of the separate launches on the same inputs: window attention
    (ir_op_swin_attention, mask computed in-kernel from the plain table) -> proj + residual -> LayerNorm -> fc1 + GELU-erf -> fc2 + residual."""
    B, H, W_, shift, C, hid, _ = CASES[case]
    w, j, x, qkv, ref = reference(case)
    T, D, d, p = B * H * W_, w.dev, w.d(j), L.ptr
    qkv_d, x_d = L.bf16_bits(qkv).cuda(), x.cuda()
    xo = torch.full((T, R.CP), float("nan"), device="cuda")
    ctx.check(run_block(ctx, w, j, shift, B, H, W_, qkv_d, x_d, xo, None, "copy"), "swin_block")
    s = ctx.stream()
    att = torch.empty(T, R.CP, dtype=torch.int16, device="cuda")
    ctx.check(ctx.lib.ir_op_swin_attention(ctx.h, s, p(qkv_d), p(att), p(D[d + "biasT"]), B, H, W_, R.HEADS, shift, w.hd ** -0.5), "swin attention")
    xa = torch.empty(T, R.CP, device="cuda")
    ctx.check(ctx.lib.ir_op_linear(ctx.h, s, p(att), p(D[d + "proj.w"]), p(D[d + "proj.b"]), p(xa), T, R.CP, R.CP, R.CP, L.ACT_NONE, None, p(x_d), 1, 1, 1.0), "proj")
    xn = torch.empty(T, R.CP, dtype=torch.int16, device="cuda")
    ctx.check(ctx.lib.ir_op_layernorm(ctx.h, s, p(xa), p(xn), p(D[d + "n2.g"]), p(D[d + "n2.b"]), T, C, R.CP, R.CP, 1e-5), "norm2")
    hb = torch.empty(T, w.hid_p, dtype=torch.int16, device="cuda")
    ctx.check(ctx.lib.ir_op_linear(ctx.h, s, p(xn), p(D[d + "fc1.w"]), p(D[d + "fc1.b"]), p(hb), T, R.CP, w.hid_p, w.hid_p, L.ACT_GELU_ERF, None, None, 0, 0, 1.0), "fc1")
    xu = torch.empty(T, R.CP, device="cuda")
    ctx.check(ctx.lib.ir_op_linear(ctx.h, s, p(hb), p(D[d + "fc2.w"]), p(D[d + "fc2.b"]), p(xu), T, w.hid_p, R.CP, R.CP, L.ACT_NONE, None, p(xa), 1, 1, 1.0), "fc2")
    torch.cuda.synchronize()
    fused, chain = xo.cpu(), xu.cpu()
    check_rows(w, fused, case)
    check_rows(w, chain, case + " unfused")
    gate(f"unfused chain {case}", chain, ref["out"], x)
    e_f, e_c = (float((o - ref["out"]).pow(2).mean().sqrt()) for o in (fused, chain))
    print(f"RMS {case}: fused {e_f:.3e}, unfused {e_c:.3e} ({e_f / e_c:.3f}x)")
    assert e_f <= 1.1 * e_c, f"{case}: fused rms error {e_f:.3e} against the unfused chain's {e_c:.3e}"


@pytest.mark.parametrize("case", ["product_s0", "product_s4", "batch_s4", "window_s4", "nopad_s4"])
def test_swin_attn_proj(ctx, case):
    """swin_attn_proj_kernel: x + proj(W-MSA) + proj bias against the reference's post-attention rows."""
    B, H, W_, shift, C, hid, _ = CASES[case]
    w, j, x, qkv, ref = reference(case)
    T, D, d, p, what = B * H * W_, w.dev, w.d(j), L.ptr, f"swin_attn_proj {case}"
    qkv_d, x_d = L.bf16_bits(qkv).cuda(), x.cuda()
    run = lambda xin, xout: ctx.lib.ir_op_swin_attn_proj(ctx.h, ctx.stream(), p(qkv_d), p(xin), p(xout), p(D[d + "proj_t"]), p(D[d + "proj.b"]),
                                                         p(D[d + ("biasM" if shift else "biasT")]), B, H, W_, shift, w.hd ** -0.5)
    outs = []
    for _ in range(2):
        xo = torch.full((T, R.CP), float("nan"), device="cuda")
        ctx.check(run(x_d, xo), what)
        outs.append(xo)
    xi = x_d.clone()
    ctx.check(run(xi, xi), what + " in place")
    torch.cuda.synchronize()
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], xi), f"{what}: repeated / in-place launches differ"
    got = outs[0].cpu()
    check_rows(w, got, what)
    gate(what, got, ref["attn"], x)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T", [4096, 1920, 1000, 1])
def test_swin_mlp(ctx, T, form):
    """swin_mlp_kernel in place (as the model runs it) on T token rows: 256 per workgroup, so 1000 and 1 leave a ragged workgroup."""
    w, j = weights(180, 360, 1.0), 0
    g = torch.Generator().manual_seed(T)
    x = torch.zeros(T, R.CP)
    x[:, :w.C] = torch.randn(T, w.C, generator=g)
    ref = R.mlp_half(w, j, x)
    D, d, n, p, what = w.dev, w.d(j), w.d(j + 1), L.ptr, f"swin_mlp T={T} {form}"
    nxt, tail = form in ("ln1", "qkv"), form == "qkv"
    x_d = x.cuda()
    res = []
    for _ in range(2):
        xi, o2 = x_d.clone(), out2_buf(T, form)
        ctx.check(ctx.lib.ir_op_swin_mlp(ctx.h, ctx.stream(), p(xi), p(xi), p(o2), p(D[d + "mlp_t"]), p(D[d + "mlp_v"]), T, w.C, w.hid_p, 1e-5,
                                         p(D[n + "n1.g"]) if nxt else None, p(D[n + "n1.b"]) if nxt else None, p(D[n + "qkv_t"]) if tail else None,
                                         p(D[n + "qkv.b"]) if tail else None, R.LDQ if tail else 0), what)
        res.append((xi, o2))
    torch.cuda.synchronize()
    assert same_bits(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), f"{what}: two launches differ"
    got = res[0][0].cpu()
    check_rows(w, got, what)
    gate(what, got, ref, x)
    check_out2(w, j, form, got, res[0][1].cpu(), what)
