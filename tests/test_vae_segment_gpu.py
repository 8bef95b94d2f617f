"""Segment-level parity of the VAE chain at product shapes: ir_op_vae_segment (the production resblock() / attnblock() / resample host code of
csrc/api.cpp on the configured, full-width VAE) against tests/support/vae_segment_ref.py evaluated with torch on the GPU.

Reference: the whole segment in fp32 (one GEMM per conv tap, no reduced-precision mode; GroupNorm statistics and the attention core in float64),
certified by float64 row bands (top, middle, bottom: 16 output rows or more plus a halo of 32 input rows) that replay the statistics and the
attention k / v of the full-size pass: the bands must agree with the fp32 pass to 1e-4 relative L2, else the case fails as "reference not
trustworthy". Nothing here reads the library under test for the reference.

Gates: R.GATES of the segment kind (derived in tests/test_vae_segment_ref_cpu.py from the bf16 / fp8 emulation, 2x margin): whole output, border
frame, last block's update. Each case also checks: a repeated launch gives the same bits; image 1 of a batch equals that image run alone; the
same segment under ir_set_plain_kernels(1) is inside the gates and the fast route's rel-L2 is at most 1.15x the plain route's; the profiler rows
pin the launch count of every conv, GroupNorm, attention and linear kernel row; an fp8 case differs from the bf16 bits and switching fp8 off restores them.

Measured on the MI355X, fast route, value (share of its gate) for rel-L2 / worst of the whole output, the border frame, the last block's update;
the plain route's figures are the same to two digits (fast / plain rel-L2 1.000 .. 1.074) and equal the GPU-side emulation to three:
    dec_l0          5.97e-3 (0.30)  3.59e-3 (0.45)  5.51e-3 (0.28)  1.80e-3 (0.45)  9.10e-3 (0.46)  1.08e-2 (0.36)
    dec_l0_fp8      6.61e-2 (0.33)  3.70e-2 (0.41)  5.92e-2 (0.30)  1.74e-2 (0.43)  1.01e-1 (0.34)  1.11e-1 (0.37)
    dec_l1          5.06e-3 (0.51)  3.14e-3 (0.45)  4.80e-3 (0.48)  1.63e-3 (0.41)  7.39e-3 (0.37)  8.84e-3 (0.44)
    dec_l32         6.98e-3 (0.35)  3.80e-3 (0.38)  6.51e-3 (0.33)  1.90e-3 (0.47)  1.11e-2 (0.37)  1.18e-2 (0.39)
    dec_l32_fp8     8.39e-2 (0.42)  4.56e-2 (0.46)  7.55e-2 (0.38)  1.75e-2 (0.44)  1.33e-1 (0.44)  1.42e-1 (0.47)
    dec_mid         4.72e-3 (0.24)  4.15e-3 (0.46)  4.18e-3 (0.21)  2.31e-3 (0.39)  7.46e-3 (0.25)  1.31e-2 (0.33)
    enc_l01         5.51e-3 (0.28)  3.49e-3 (0.50)  5.27e-3 (0.26)  2.12e-3 (0.42)  8.37e-3 (0.42)  1.05e-2 (0.53)
    enc_l01_fp8     6.58e-2 (0.33)  3.73e-2 (0.41)  6.09e-2 (0.30)  2.24e-2 (0.37)  9.98e-2 (0.33)  1.12e-1 (0.37)
    enc_l23mid      5.60e-3 (0.28)  3.97e-3 (0.50)  5.23e-3 (0.26)  2.24e-3 (0.37)  6.84e-2 (0.34)  6.47e-2 (0.32)
    tiles_dec_l0    5.94e-3 (0.30)  3.39e-3 (0.42)  5.54e-3 (0.28)  1.90e-3 (0.48)  9.20e-3 (0.46)  8.84e-3 (0.29)
    tiles_dec_mid   5.57e-3 (0.28)  4.52e-3 (0.50)  4.88e-3 (0.24)  2.86e-3 (0.48)  9.09e-3 (0.30)  1.61e-2 (0.40)
    ragged_dec_l0   5.91e-3 (0.30)  3.62e-3 (0.45)  5.51e-3 (0.28)  1.57e-3 (0.39)  9.08e-3 (0.45)  1.08e-2 (0.36)
    ragged_dec_l32  7.07e-3 (0.35)  3.94e-3 (0.39)  6.49e-3 (0.32)  1.68e-3 (0.42)  1.11e-2 (0.37)  1.10e-2 (0.37)
    ragged_enc_l01  5.48e-3 (0.27)  3.21e-3 (0.46)  5.22e-3 (0.26)  2.07e-3 (0.41)  8.39e-3 (0.42)  9.39e-3 (0.47)
    small_dec_l32   7.47e-3 (0.37)  4.37e-3 (0.44)  6.95e-3 (0.35)  2.11e-3 (0.53)  1.15e-2 (0.38)  1.17e-2 (0.39)
    peaky_dec_mid   3.62e-2 (0.52)  2.08e-1 (0.52)  5.08e-2 (0.25)  1.89e-1 (0.47)  3.21e-1 (0.46)  3.85e+0 (0.55)   one launch on the fallback
Some `worst` figures sit at gate / 2 on the plain kernels too, so the gates were checked against the emulation at these very sizes (see GATES
in the support module). The whole file takes about 25 s on the MI355X; no case takes more than 5 s (the largest share: host-side generation
of the 2048 x 2048 inputs and the fp32 reference pass).
"""
from contextlib import contextmanager
from functools import lru_cache
import ctypes as C
import time

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import vae_segment_ref as R

pytestmark = pytest.mark.gpu

FAST_OVER_PLAIN = 1.15
HALO, CORE = 32, 16
K_S1, K_PP, K_HALO, K_IGEMM9 = "conv3x3/conv_halo_s1_kernel", "conv3x3/conv_halo_pp_kernel", "conv3x3/conv_halo_kernel", "conv3x3/igemm_kernel<taps=9>"
K_S1_FP8, K_HALO_FP8 = "conv3x3/conv_halo_s1_fp8_kernel", "conv3x3/conv_halo_kernel<.., fp8>"
K_GN_FUSED, K_GN_OWN = "groupnorm/gn_finalize_groups+gn_apply (statistics from the conv epilogue)", "groupnorm/gn_partial+gn_finalize+gn_apply"
K_ATTN, K_ATTN_FP8 = "flash_attn/flash_attn_d512_v2_kernel (VAE mid-block)", "flash_attn/flash_attn_d512_fp8_kernel (VAE mid-block, fp8 operands)"
K_LIN, K_GEMM_PP = "linear/igemm_kernel<taps=1>", "linear/gemm_pp_kernel"
# every case pins the launch count of EACH of these rows on the fast route (a row a case does not list must not launch at all)
PINNED = (K_S1, K_PP, K_HALO, K_IGEMM9, K_S1_FP8, K_HALO_FP8, K_GN_FUSED, K_GN_OWN, K_ATTN, K_ATTN_FP8, K_LIN, K_GEMM_PP)


def rows(s1=0, pp=0, halo=0, igemm9=0, s1_fp8=0, gn_fused=0, gn_own=0, attn=0, attn_fp8=0, lin=0):
    return {K_S1: s1, K_PP: pp, K_HALO: halo, K_IGEMM9: igemm9, K_S1_FP8: s1_fp8, K_HALO_FP8: 0, K_GN_FUSED: gn_fused, K_GN_OWN: gn_own, K_ATTN: attn,
            K_ATTN_FP8: attn_fp8, K_LIN: lin, K_GEMM_PP: 0}


# id: segment kind, images n, input size h x w of the segment's first step, weights, fp8 (True: every mask bit; "attn": the attention bits
# alone), launches of the fast route per pinned row. What the counts say:
#  * gn_own = GroupNorms on the stand-alone statistics pass: the first block of a segment that starts with a block, the block behind the
#    attention (mid.res1: stale gn_chunks around, no gn_x) - and, in the small case, one more: at n = 2 and 16 x 24 one conv cannot write
#    partials (a 128-row tile would straddle the images), so its consumer falls back. gn_fused = every other GroupNorm.
#  * the small case runs below 32 patch tiles: conv_halo_pp / conv_halo, no conv_halo_s1 at all.
#  * igemm9 = the stride-2 Downsample conv; lin = the shortcut linear and the attention's q / k / v / proj_out.
#  * The rows cannot tell the NORM form of conv_halo_s1 (norm1 / norm2 folded into the conv, taken for cout_pad == 128) from the plain conv
#    behind a fused apply pass: both are one gn_fused and one s1 launch. Dropping the NORM route would change bits (the fast / plain ratio and the
#    gates see the values), not these counts.
# The peaky case runs with fp8 ATTENTION operands: the bf16 d = 512 kernel moves its softmax reference in place and cannot be made to raise its
# overflow flag by any scores, so the way into attnblock()'s fallback chain is the fp8 kernel's flag ("a query I cannot handle"), behind which
# the bf16 d = 512 kernel recomputes the whole launch: the case asserts that the result then has the bits of the bf16 route. The 4-wave
# rescaling pair at the END of the chain (behind the bf16 kernel's own flag) is NOT reached by this or any other case. The chain is attn_d512() of
# csrc/api.cpp; ir_op_attention and ir_op_attention_d512_fp8 run the same function (tests/test_attn_routes_gpu.py holds both to the same bits).
CASES = {
    "dec_l0": ("dec_l0", 1, 1024, 1024, "base", False, rows(s1=7, gn_fused=6, lin=1)),
    "dec_l0_fp8": ("dec_l0", 1, 1024, 1024, "base", True, rows(s1=1, s1_fp8=6, gn_fused=6, lin=1)),
    "dec_l1": ("dec_l1", 1, 512, 512, "base", False, rows(s1=5, gn_fused=4, lin=1)),
    "dec_l32": ("dec_l32", 1, 256, 256, "base", False, rows(s1=11, gn_fused=9, gn_own=1)),
    "dec_l32_fp8": ("dec_l32", 1, 256, 256, "base", True, rows(s1=1, s1_fp8=10, gn_fused=9, gn_own=1)),
    "dec_mid": ("dec_mid", 1, 256, 256, "base", False, rows(s1=4, gn_fused=3, gn_own=2, attn=1, lin=4)),
    "enc_l01": ("enc_l01", 1, 2048, 2048, "base", False, rows(s1=6, igemm9=1, gn_fused=5, gn_own=1, lin=1)),
    "enc_l01_fp8": ("enc_l01", 1, 2048, 2048, "base", True, rows(s1_fp8=6, igemm9=1, gn_fused=5, gn_own=1, lin=1)),
    "enc_l23mid": ("enc_l23mid", 1, 512, 512, "base", False, rows(s1=6, igemm9=1, gn_fused=7, attn=1, lin=4)),
    "tiles_dec_l0": ("dec_l0", 4, 256, 256, "base", False, rows(s1=7, gn_fused=6, lin=1)),
    "tiles_dec_mid": ("dec_mid", 4, 64, 64, "base", False, rows(s1=4, gn_fused=3, gn_own=2, attn=1, lin=4)),
    "ragged_dec_l0": ("dec_l0", 1, 544, 552, "base", False, rows(s1=7, gn_fused=6, lin=1)),
    "ragged_dec_l32": ("dec_l32", 1, 136, 138, "base", False, rows(s1=11, gn_fused=9, gn_own=1)),
    "ragged_enc_l01": ("enc_l01", 1, 1088, 1104, "base", False, rows(s1=6, igemm9=1, gn_fused=5, gn_own=1, lin=1)),
    "small_dec_l32": ("dec_l32", 2, 16, 24, "base", False, rows(pp=10, halo=1, gn_fused=8, gn_own=2)),
    "peaky_dec_mid": ("dec_mid", 1, 64, 64, "peaky", "attn", rows(s1=4, gn_fused=3, gn_own=2, attn=1, attn_fp8=1, lin=4)),
}


@contextmanager
def full_precision():
    """No TF32 / reduced-precision products inside the reference."""
    mm, cd = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    prec = torch.get_float32_matmul_precision()
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = mm, cd
        torch.set_float32_matmul_precision(prec)


@lru_cache(maxsize=None)
def model(wkind):
    from instarevive_amd.models import AutoencoderKL
    m = AutoencoderKL(block_out_channels=(128, 256, 512, 512))
    m.load_state_dict(R.weights(wkind), strict=True)
    return m.to("cuda")


def info(ctx, half):
    """[(name, cin, cout)] of the half's steps, from the library."""
    count = ctx.lib.ir_op_vae_segment_info(ctx.h, half, -1, 0, 0, None, 0, None, None, None, None)
    assert count > 0, count
    out = []
    for i in range(count):
        name = C.create_string_buffer(32)
        cin, cout, oh, ow = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        assert ctx.lib.ir_op_vae_segment_info(ctx.h, half, i, 8, 8, name, 32, C.byref(cin), C.byref(cout), C.byref(oh), C.byref(ow)) == count
        out.append((name.value.decode(), cin.value, cout.value, oh.value, ow.value))
    return out


def out_shape(ctx, half, first, count, h, w):
    cout = 0
    for i in range(first, first + count):
        co, oh, ow = C.c_int(), C.c_int(), C.c_int()
        ctx.lib.ir_op_vae_segment_info(ctx.h, half, i, h, w, None, 0, None, C.byref(co), C.byref(oh), C.byref(ow))
        h, w, cout = oh.value, ow.value, co.value
    return cout, h, w


def launch(m, half, first, count, x_nhwc):
    """ir_op_vae_segment on x [n][h][w][c] bf16 (device): (return code, y [n][oh][ow][cout] bf16)."""
    ctx = m.ctx
    n, h, w, _ = x_nhwc.shape
    cout, oh, ow = out_shape(ctx, half, first, count, h, w)
    y = torch.empty(n, max(oh, 0), max(ow, 0), cout, dtype=torch.bfloat16, device="cuda")
    ws = ctx.workspace(max(int(ctx.lib.ir_op_vae_segment_ws(ctx.h, half, first, count, n, h, w)), 256))
    rc = ctx.lib.ir_op_vae_segment(ctx.h, ctx.stream(), half, first, count, L.ptr(x_nhwc), L.ptr(y), n, h, w, L.ptr(ws), ws.numel())
    return rc, y


def run(m, half, first, count, x_nhwc, what):
    rc, y = launch(m, half, first, count, x_nhwc)
    m.ctx.check(rc, what)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), what
    return y


def bands(H, core):
    """Input-row bands [a, b) (bounds multiples of 4) of an H-row map: top, middle, bottom with `core` certified rows each - or the whole map
    when it is small."""
    if H <= 3 * (core + 2 * HALO):
        return [(0, H)]
    mid = (H // 2) & ~3
    return [(0, core + HALO), (mid - HALO, mid + core + HALO), (H - core - HALO, H)]


@lru_cache(maxsize=1)
def reference(kind, n, h, w, wkind):
    """(x NCHW fp32 on the CPU, reference output and last-step skip path fp32 on the GPU), certified by float64 row bands."""
    sd = R.weights(wkind)
    half, first, count = R.span(kind)
    x = R.make_input(n, R.in_channels(sd, half, first), h, w, seed=n * h * w + first, gain=R.input_scale(half, first), spike=wkind == "peaky")
    t0 = time.time()
    with full_precision():
        tape = R.Tape()
        ref, skip = R.segment(sd, half, first, count, x.cuda(), tape=tape)
        torch.cuda.synchronize()
        t1 = time.time()
        s = ref.shape[2] / h   # output rows per input row
        for a, b in bands(h, int(CORE / min(s, 1.0))):
            tape.rewind()
            band, _ = R.segment(sd, half, first, count, x[:, :, a:b].cuda().double(), tape=tape)
            lo = a if a == 0 else a + HALO
            hi = b if b == h else b - HALO
            r0, r1 = int(lo * s), int(hi * s)
            got, want = ref[:, :, r0:r1].double(), band[:, :, r0 - int(a * s):r1 - int(a * s)]
            err = float((got - want).norm() / want.norm())
            print(f"CERT {kind} n{n} {h}x{w}: rows {r0}..{r1 - 1} fp32 pass vs float64 band {err:.1e}")
            assert r1 - r0 >= min(CORE, ref.shape[2]) and err <= 1e-4, f"reference not trustworthy: {kind} rows {r0}..{r1}: {err:.2e}"
            del band, got, want
    torch.cuda.synchronize()
    print(f"TIME {kind} n{n} {h}x{w}: reference fp32 pass {t1 - t0:.1f} s, float64 bands {time.time() - t1:.1f} s")
    del tape
    torch.cuda.empty_cache()
    return x, ref, skip


_resident = [None]


def gate(what, y, ref, skip, gk):
    e = R.errors(y.permute(0, 3, 1, 2).float(), ref, skip)
    g = R.GATES[gk]
    print(f"MEASURED {what}: " + "  ".join(f"{k} {e[k]:.2e} ({e[k] / g[k]:.2f} of gate)" for k in e))
    for k in e:
        assert e[k] <= g[k], f"{what}: {k} {e[k]:.3e} exceeds its gate {g[k]:.0e}"
    return e["l2"]


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("case", list(CASES))
def test_vae_segment(case):
    kind, n, h, w, wkind, fp8, routes = CASES[case]
    t_start = time.time()
    m = model(wkind)
    m._ready()
    ctx = m.ctx
    half, first, count = R.span(kind)
    names = [s[0] for s in R.steps(half)]
    assert [i[0] for i in info(ctx, half)] == names, "the library's step table and the reference's disagree"
    key = (kind, n, h, w, wkind)
    if _resident[0] != key:   # one case resident at a time: the previous reference goes before the next is made
        reference.cache_clear()
        torch.cuda.empty_cache()
        _resident[0] = key
    x, ref, skip = reference(*key)
    xd = x.cuda().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    gk = kind + ("_peaky" if wkind == "peaky" else "") + ("_fp8" if fp8 is True else "")
    what = f"vae segment {case} ({names[first]} .. {names[first + count - 1]}, n {n}, {h} x {w})"
    try:
        if fp8:
            plain_bits = run(m, half, first, count, xd, what + " bf16")
            m.enable_fp8(True)
            ctx.check(ctx.lib.ir_set_fp8_mask(ctx.h, L.FP8_MASK_ALL if fp8 is True else L.FP8_MASK_ATTENTION), "ir_set_fp8_mask")
        a = run(m, half, first, count, xd, what)
        ctx.profile_begin()
        if wkind == "peaky":
            ctx.check(ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 1), "ir_attn_fallback_count")
        b = run(m, half, first, count, xd, what + " again")
        if wkind == "peaky":
            fb = ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), 0)
            ctx.check(ctx.lib.ir_attn_fallback_count(ctx.h, ctx.stream(), -1), "ir_attn_fallback_count")
            print(f"{what}: {fb} attention launch(es) took the fallback")
            assert fb > 0, f"{what}: the scores never outgrew the fixed softmax reference - the case does not reach the fallback"
        launched = ctx.profile_end_kernels()
        print(f"ROWS {what}: " + ", ".join(f"{k} x{v['launches']}" for k, v in sorted(launched.items())))
        assert same(a, b), f"{what}: two launches differ"
        assert set(routes) == set(PINNED)
        wrong = {k: (launched.get(k, {}).get("launches", 0), cnt) for k, cnt in routes.items() if launched.get(k, {}).get("launches", 0) != cnt}
        assert not wrong, f"{what}: launches (got, expected) {wrong}"
        l2_fast = gate(what, a, ref, skip, gk)
        if fp8:
            if fp8 is True:
                assert not same(a, plain_bits), f"{what}: fp8 on gives the bf16 bits - the fp8 branch did not run"
            else:   # the fallback recomputed EVERY query with the bf16 kernel on the same q / k / V^T tiles
                assert same(a, plain_bits), f"{what}: behind the fp8 kernel's flag the result is not the bf16 route's, bit for bit"
            m.enable_fp8(False)
            assert same(run(m, half, first, count, xd, what + " fp8 off"), plain_bits), f"{what}: switching fp8 off does not restore the bf16 bits"
            m.enable_fp8(True)
        if n > 1:   # image 1 alone
            solo = run(m, half, first, count, xd[1:2].contiguous(), what + " image 1 alone")
            assert same(a[1:2], solo), f"{what}: image 1 of the batch differs from image 1 run alone"
        try:   # the same segment on the plain (4-wave) kernels
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
            c = run(m, half, first, count, xd, what + " plain")
        finally:
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
        l2_plain = gate(what + " plain", c, ref, skip, gk)
        print(f"RATIO {what}: fast / plain rel-L2 {l2_fast / l2_plain:.3f}; case wall time {time.time() - t_start:.1f} s")
        assert l2_fast <= FAST_OVER_PLAIN * l2_plain, f"{what}: fast route rel-L2 {l2_fast:.3e} against the plain route's {l2_plain:.3e}"
    finally:
        if fp8:
            ctx.check(ctx.lib.ir_set_fp8_mask(ctx.h, L.FP8_MASK_DEFAULT), "ir_set_fp8_mask")
            m.enable_fp8(False)
        ctx._ws = None
        del xd
        torch.cuda.empty_cache()


def test_vae_segment_refuses_bad_arguments():
    """-1 for a bad half, first or count or a null tensor; -10 for n < 1, an empty map or an odd size in front of a Downsample; -20 for a
    workspace that is too small; -11 when the half is not configured. The output buffer stays untouched."""
    m = model("base")
    m._ready()
    ctx = m.ctx
    nd, ne = len(R.steps(1)), len(R.steps(0))
    x = torch.zeros(1, 8, 8, 512, dtype=torch.bfloat16, device="cuda")

    def rc(half, first, count, n=1, h=8, w=8, ws_bytes=None, xin=x):
        y = torch.full((1, 16, 16, 512), 7.0, dtype=torch.bfloat16, device="cuda")
        ws = ctx.workspace(1 << 26)
        r = ctx.lib.ir_op_vae_segment(ctx.h, ctx.stream(), half, first, count, L.ptr(xin), L.ptr(y), n, h, w, L.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) or r == 0, "a refused call wrote to the output"
        return r

    assert rc(1, 0, 1) == 0
    for half, first, count in ((2, 0, 1), (-1, 0, 1), (1, -1, 1), (1, 0, 0), (1, nd, 1), (1, nd - 1, 2), (0, ne - 2, 3)):
        assert rc(half, first, count) == -1, (half, first, count)
    assert rc(1, 0, 1, xin=None) == -1
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -8)):
        assert rc(1, 0, 1, n, h, w) == -10, (n, h, w)
    ds = [s[0] for s in R.steps(0)].index("down2.ds")
    assert rc(0, ds, 1, 1, 7, 8) == -10 and rc(0, ds, 1, 1, 8, 7) == -10 and rc(0, ds - 1, 2, 1, 7, 8) == -10
    assert ctx.lib.ir_op_vae_segment_ws(ctx.h, 0, ds, 1, 1, 7, 8) == 0
    assert rc(1, 0, 1, ws_bytes=4096) == -20
    bare = L.Context(0)
    assert bare.lib.ir_op_vae_segment(bare.h, bare.stream(), 1, 0, 1, L.ptr(x), L.ptr(x), 1, 8, 8, None, 0) == -11
    assert bare.lib.ir_op_vae_segment_info(bare.h, 1, -1, 0, 0, None, 0, None, None, None, None) == -11
