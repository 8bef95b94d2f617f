"""Segment-level parity of the SwinIR shell around its blocks: ir_op_swin_shell (the production swin_head() / swin_rstb_tail() / swin_recon() host
code of csrc/api.cpp, which swinir_run() calls around its block loop) on the configured full-width model against tests/support/swin_shell_ref.py
evaluated in float64 with torch on the GPU. Nothing here reads the library under test for the reference.

Cases are the smallest sizes at which a route or an edge exists (see CASES). Gates: R.gates(case, key), derived in
tests/test_swin_shell_ref_cpu.py from the emulation of the path's number formats (2x margin); every case re-measures that emulation in float64
at its own size and asserts that it stays under half of each gate. Each case also checks: the plain route (ir_set_plain_kernels(1)) is inside
the gates and the fast route's rel-L2 is at most 1.15x the plain route's; a repeated launch gives the same bits; image 1 of a batch equals that
image run alone; the profiler rows of the part; the workspace is exactly ir_op_swin_shell_ws bytes, pre-filled with 0xFF bytes (NaN in bf16 and
fp32), and one byte less is refused with -20 before anything is launched; canaries behind every output are untouched; the pad columns 180 .. 191
of the token outputs are exactly zero.

What the profiler rows can and cannot tell: the three nearest-2x convs run on conv_halo_kernel in their phase form (fast route, when the host
packed swin.up*.wup - asserted) and in the 9-tap form (plain route) alike, one row for both. That the phase form ran is seen in the bits: the
fast and the plain reconstruction differ at the sizes where nothing else differs between the routes (192 x 320, 512 x 1024).

Measured figures: docs/parity.md, section "SwinIR shell".
"""
from contextlib import contextmanager
from functools import lru_cache
import time

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import swin_shell_ref as R

pytestmark = pytest.mark.gpu

FAST_OVER_PLAIN = 1.15
K_HALO, K_IGEMM9, K_LN, K_OTHER = "conv3x3/conv_halo_kernel", "conv3x3/igemm_kernel<taps=9>", "layernorm/layernorm_*_kernel", "other/layout+glue"
K_TO3 = "conv3x3/vae_norm_conv_out_kernel<1, false> (SwinIR conv_last 64->3, read-bound)"
CANARY, TAIL = -1234.5, 4096

# id: part, RSTB layer, images, pixels h x w. What each size is there for:
#  64 x 64        one 8 x 16 halo tile, partly empty; 64 token rows: the layernorm_v4 route; the smallest reconstruction
#  192 x 320 (2)  token grid 24 x 40: a ragged tile column (at every one of the four resolutions of the reconstruction), two images
#  512 x 1024     64 x 128 tokens = 64 tiles, where tile_grid() switches to the XCD-padded order; 8192 rows: the layernorm_r16 route (from 4096);
#                 the generic conv_last (Cout = 3, scalar stores into rows of 4) on a large grid
#  1024 x 1024    the smallest frame whose conv_last runs on ir_launch_conv64_to3
SIZES = {"64x64": (1, 64, 64), "192x320x2": (2, 192, 320), "512x1024": (1, 512, 1024), "1024x1024": (1, 1024, 1024)}
CASES = {}
for _s in ("64x64", "192x320x2", "512x1024"):
    CASES[f"head_{_s}"] = ("head", 0) + SIZES[_s]
    for _l in (0, 1):
        CASES[f"tail{_l}_{_s}"] = ("rstb_tail", _l) + SIZES[_s]
for _s in SIZES:
    CASES[f"recon_{_s}"] = ("recon", 0) + SIZES[_s]
PART = {"head": R.HEAD, "rstb_tail": R.RSTB_TAIL, "recon": R.RECON}


def expected_rows(part, h, w, plain):
    """Launches per profiler row of one part."""
    if part == "head":       # swin_prep, conv_first, patch-embed LayerNorm
        return {K_OTHER: 1, K_HALO: 1, K_LN: 1}
    if part == "rstb_tail":
        return {K_HALO: 1}
    to3 = not plain and h * w >= 1024 * 1024
    # final LayerNorm; conv_after_body, before_up, up1..3, hr; conv_last; nhwc_to_nchw
    return {K_LN: 1, K_HALO: 6, (K_TO3 if to3 else K_IGEMM9): 1, K_OTHER: 1}


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
def model():
    return R.model()


def guarded(shape, dtype, fill):
    """(tensor of `shape` filled with `fill`, the canary tail behind it), one allocation."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + TAIL,), CANARY, dtype=dtype, device="cuda")
    flat[:n] = fill
    return flat[:n].view(shape), flat[n:]


def inputs(part, layer, n, h, w):
    """The part's input tensors on the CPU (fp32 values; xc bf16-exact)."""
    gh, gw = h // 8, w // 8
    seed = n * h * w + 7 * layer
    if part == "head":
        return (R.make_image(n, h, w, seed),)
    if part == "rstb_tail":
        return R.make_tokens(n, gh, gw, seed + 1, bf16=True, gain=R.GAIN["xc"]), R.make_tokens(n, gh, gw, seed + 2, gain=R.GAIN["xa_tail"])
    return R.make_tokens(n, gh, gw, seed + 3, gain=R.GAIN["xa_recon"]), R.make_tokens(n, gh, gw, seed + 4, gain=R.GAIN["x0"])


def launch(m, part, layer, ins, n, h, w, short=0, what=""):
    """ir_op_swin_shell on device inputs: (return code, outputs). The workspace holds exactly ir_op_swin_shell_ws bytes (less `short`) of
    0xFF; the canaries behind the outputs are checked here, and that a refused call left the outputs as they were."""
    ctx = m.ctx
    T = n * (h // 8) * (w // 8)
    need = int(ctx.lib.ir_op_swin_shell_ws(ctx.h, PART[part], n, h, w))
    assert need > 0, what
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    nan = float("nan")
    if part == "head":
        (x0, t0), (xa, t1) = guarded((T, R.CP), torch.float32, nan), guarded((T, R.CP), torch.float32, nan)
        args, outs, tails = (L.ptr(ins[0]), None, L.ptr(x0), L.ptr(xa)), (x0, xa), (t0, t1)
    elif part == "rstb_tail":
        xa, t0 = guarded((T, R.CP), torch.float32, nan)
        xa.copy_(ins[1])
        args, outs, tails = (L.ptr(ins[0]), None, L.ptr(xa), None), (xa,), (t0,)
    else:
        y, t0 = guarded((n, 3, h, w), torch.float32, nan)
        args, outs, tails = (L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(y), None), (y,), (t0,)
    before = [o.clone() for o in outs]
    rc = ctx.lib.ir_op_swin_shell(ctx.h, ctx.stream(), PART[part], layer, *args, n, h, w, L.ptr(ws), need - short)
    torch.cuda.synchronize()
    for t in tails:
        assert bool((t == CANARY).all()), f"{what}: wrote behind an output"
    if rc != 0:
        for o, b in zip(outs, before):
            assert same(o, b), f"{what}: a refused call (rc {rc}) wrote to an output"
    return rc, outs


def run(m, part, layer, ins, n, h, w, what):
    rc, outs = launch(m, part, layer, ins, n, h, w, what=what)
    m.ctx.check(rc, what)
    for o in outs:
        assert torch.isfinite(o).all(), f"{what}: an output element was not written (or is not finite)"
    return outs


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def measure(case, part, outs, ref, ins64, n, h, w):
    """{gate key: errors} of a part's outputs against the reference."""
    gh, gw = h // 8, w // 8
    if part == "head":
        return {"head_x0": R.token_errors(outs[0], ref[0], n, gh, gw), "head_xa": R.token_errors(outs[1], ref[1], n, gh, gw)}
    if part == "rstb_tail":
        return {"rstb_tail": R.token_errors(outs[0], ref[0], n, gh, gw, base=ins64[1])}
    return {"recon": R.errors(outs[0], ref[0], 8)}


def reference(part, layer, ins64, n, h, w, emulate=False):
    gh, gw = h // 8, w // 8
    sd = R.weights()
    if part == "head":
        return R.head(sd, ins64[0], emulate=emulate)
    if part == "rstb_tail":
        return (R.rstb_tail(sd, layer, ins64[0], ins64[1], n, gh, gw, emulate=emulate),)
    return (R.recon(sd, ins64[0], ins64[1], n, gh, gw, emulate=emulate),)


def gate(case, what, e, problems, half=False):
    """Prints every figure with its share of the gate and notes those outside in `problems` (the case asserts at its end, so that one run
    shows every figure); -> the largest rel-L2."""
    for key, ek in e.items():
        g = R.gates(case, key)
        print(f"MEASURED {what} {key}: " + "  ".join(f"{k} {ek[k]:.2e} ({ek[k] / g[k]:.2f} of gate)" for k in ek))
        for k in ek:
            if not ek[k] <= (g[k] / 2 if half else g[k]):
                problems.append(f"{what} {key}: {k} {ek[k]:.3e} exceeds {'half of ' if half else ''}its gate {g[k]:.0e}")
    return max(ek["l2"] for ek in e.values())


@pytest.mark.parametrize("case", list(CASES))
def test_swin_shell(case):
    part, layer, n, h, w = CASES[case]
    t_start = time.time()
    m = model()
    m._ready()
    ctx = m.ctx
    assert ctx.has("swin.up1.wup") and ctx.has("swin.up2.wup") and ctx.has("swin.up3.wup"), "the host did not pack the phase forms of the up-convs"
    what = f"swin shell {case}"
    cpu = inputs(part, layer, n, h, w)
    ins64 = [t.cuda().double() for t in cpu]
    dev = [t.cuda() for t in cpu]
    if part == "rstb_tail":
        dev[0] = dev[0].to(torch.bfloat16)
        assert torch.equal(dev[0].float(), cpu[0].cuda()), "xc is not bf16-exact"
    with full_precision():
        ref = reference(part, layer, ins64, n, h, w)
        emu = reference(part, layer, ins64, n, h, w, emulate=True)
        torch.cuda.synchronize()
    t_ref = time.time() - t_start
    problems = []
    gate(case, what + " EMULATION", measure(case, part, emu, ref, ins64, n, h, w), problems, half=True)
    del emu

    a = run(m, part, layer, dev, n, h, w, what)
    ctx.profile_begin()
    b = run(m, part, layer, dev, n, h, w, what + " again")
    launched = {k: v["launches"] for k, v in ctx.profile_end_kernels().items()}
    print(f"ROWS {what}: " + ", ".join(f"{k} x{v}" for k, v in sorted(launched.items())))
    assert all(same(x, y) for x, y in zip(a, b)), f"{what}: two launches differ"
    assert launched == expected_rows(part, h, w, False), f"{what}: launches {launched}, expected {expected_rows(part, h, w, False)}"
    if part != "recon":   # the pad columns of the token rows
        for o in a:
            assert bool((o[:, R.C:] == 0).all()), f"{what}: columns 180 .. 191 are not exactly zero"
    l2_fast = gate(case, what, measure(case, part, a, ref, ins64, n, h, w), problems)

    rc, _ = launch(m, part, layer, dev, n, h, w, short=1, what=what + " workspace one byte short")
    assert rc == -20, rc

    if n > 1:   # image 1 alone
        T1 = (h // 8) * (w // 8)
        solo_in = [t[1:2].contiguous() if t.dim() == 4 else t[T1:2 * T1].contiguous() for t in dev]
        solo = run(m, part, layer, solo_in, 1, h, w, what + " image 1 alone")
        for o, s in zip(a, solo):
            o1 = o[1:2] if o.dim() == 4 else o[T1:2 * T1]
            assert same(o1.contiguous(), s), f"{what}: image 1 of the batch differs from image 1 run alone"

    try:   # the same part on the plain kernels
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        ctx.profile_begin()
        c = run(m, part, layer, dev, n, h, w, what + " plain")
        launched = {k: v["launches"] for k, v in ctx.profile_end_kernels().items()}
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
    print(f"ROWS {what} plain: " + ", ".join(f"{k} x{v}" for k, v in sorted(launched.items())))
    assert launched == expected_rows(part, h, w, True), f"{what} plain: launches {launched}, expected {expected_rows(part, h, w, True)}"
    l2_plain = gate(case, what + " plain", measure(case, part, c, ref, ins64, n, h, w), problems)
    if part == "recon" and case in ("recon_192x320x2", "recon_512x1024"):
        # nothing but the form of the three up-convs differs between the routes here: equal bits would mean that the phase form did not run
        assert not same(a[0], c[0]), f"{what}: the fast route gives the plain route's bits - the phase-form up-convs did not run"
    print(f"RATIO {what}: fast / plain rel-L2 {l2_fast / l2_plain:.3f}; reference + emulation {t_ref:.1f} s, case wall time {time.time() - t_start:.1f} s")
    assert not problems, "; ".join(problems)
    assert l2_fast <= FAST_OVER_PLAIN * l2_plain, f"{what}: fast route rel-L2 {l2_fast:.3e} against the plain route's {l2_plain:.3e}"
    del ref, ins64, dev, a, b, c
    torch.cuda.empty_cache()


def test_swin_shell_refuses_bad_arguments():
    """-1 for a bad part, a layer the model has not, or a missing tensor; -10 for a size that is no multiple of 64; -20 for a workspace that
    is too small; -11 on a context without SwinIR. Nothing is written then."""
    m = model()
    m._ready()
    ctx = m.ctx
    n, h, w = 1, 64, 64
    T = 64
    img = torch.rand(1, 3, 128, 128, device="cuda")
    xc = torch.zeros(4 * T, R.CP, dtype=torch.bfloat16, device="cuda")
    ws = torch.full((1 << 24,), 255, dtype=torch.uint8, device="cuda")

    def rc(part, layer=0, in0=img, in1=img, n=n, h=h, w=w, ws_bytes=ws.numel(), out1=True, c=ctx):
        o0 = torch.full((4 * T * R.CP,), CANARY, device="cuda")
        o1 = torch.full((4 * T * R.CP,), CANARY, device="cuda")
        r = c.lib.ir_op_swin_shell(c.h, c.stream(), part, layer, L.ptr(in0), L.ptr(in1), L.ptr(o0), L.ptr(o1) if out1 else None, n, h, w, L.ptr(ws), ws_bytes)
        torch.cuda.synchronize()
        assert r == 0 or bool((o0 == CANARY).all() and (o1 == CANARY).all()), "a refused call wrote to an output"
        return r

    assert rc(R.HEAD) == 0 and rc(R.RSTB_TAIL, 1, in0=xc) == 0
    assert rc(3) == -1 and rc(-1) == -1
    assert rc(R.RSTB_TAIL, 2, in0=xc) == -1 and rc(R.RSTB_TAIL, -1, in0=xc) == -1
    assert rc(R.HEAD, in0=None) == -1 and rc(R.HEAD, out1=False) == -1 and rc(R.RECON, in1=None) == -1
    assert rc(R.HEAD, h=96) == -10 and rc(R.HEAD, w=0) == -10 and rc(R.RECON, n=0) == -10
    assert ctx.lib.ir_op_swin_shell_ws(ctx.h, R.HEAD, 1, 96, 64) == 0 and ctx.lib.ir_op_swin_shell_ws(ctx.h, 3, 1, 64, 64) == 0
    assert rc(R.HEAD, ws_bytes=4096) == -20 and rc(R.RECON, in0=xc.float(), in1=xc.float(), ws_bytes=1 << 16) == -20
    bare = L.Context(0)
    assert rc(R.HEAD, c=bare) == -11 and rc(R.RECON, c=bare) == -11
    assert bare.lib.ir_op_swin_shell_ws(bare.h, R.HEAD, 1, 64, 64) == 0
