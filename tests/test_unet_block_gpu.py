"""Block-level parity of the ControlLDM UNet at full width: ir_op_unet_block (the production unet_update_timestep() + ublock() of csrc/api.cpp,
with cldm_run()'s scratch sizing and split-K scope) against the float64 restatement in tests/support/unet_block_ref.py, evaluated on the GPU
(attention chunked by query blocks, TF32 off).

One UNet of configs/cldm.yaml's dimensions (320 x (1, 2, 4, 4), 2 res blocks per level, heads of 64, context 1024 x 77) with det_state_dict
weights is uploaded once per module; the cases are unet_block_ref.CASES: every distinct block shape once on 8 x 8, the token counts of a 512-px
image (4096 x 320, 1024 x 640, 256 x 1280), a ragged 12 x 20 grid and two batches. Every case asserts: the output inside the gates of its block
kind (unet_block_ref.GATES = 2 x the bf16 emulation, derived by tests/test_unet_block_ref_cpu.py, which also shows that the planted bugs land
outside them); the bf16 emulation re-measured here, at the case's own size, under half of each gate; the plain route (ir_set_plain_kernels(1))
inside the gates and the fast route's rel-L2 at most 1.15 x the plain route's; a repeated launch gives the same bits; the workspace is exactly
ir_op_unet_block_ws bytes of 0xFF; `out` has out_cs = cout + 64 with canary columns and a canary tail that stay bit-untouched (the slice write
of the decoder's never-materialised concatenations); the profiler rows of ROUTES; item 1 of a batch equals that item run alone, bit for bit.

Measured on the MI355X (fast route: rel-L2 / worst of the output, then of the update where the kind has one; the plain route's figures are the
same to three digits on every case, ratio 1.000; every figure is 0.28 .. 0.59 of its gate and equals the emulation's to two digits):
    in0_conv               1.66e-3 / 1.99e-3                         in1_xf320              4.84e-3 / 4.90e-3, 6.63e-3 / 7.19e-3
    in4_320to640_xf        5.15e-3 / 6.65e-3, 6.81e-3 / 8.48e-3      in5_xf640              4.86e-3 / 4.89e-3, 6.51e-3 / 5.40e-3
    in7_640to1280_xf       5.17e-3 / 5.65e-3, 6.92e-3 / 7.83e-3      in8_xf1280             4.89e-3 / 5.38e-3, 6.55e-3 / 6.23e-3
    in10_res1280           2.16e-3 / 3.34e-3, 4.74e-3 / 6.25e-3      in3_down320            1.63e-3 / 1.90e-3
    in6_down640            1.67e-3 / 1.64e-3                         in9_down1280           1.66e-3 / 2.83e-3
    mid0_res               2.15e-3 / 3.41e-3, 4.69e-3 / 6.04e-3      mid1_xf                4.11e-3 / 4.52e-3, 5.26e-3 / 5.14e-3
    mid2_res               2.16e-3 / 3.16e-3, 4.71e-3 / 6.58e-3      out0_2560to1280        2.64e-3 / 4.39e-3
    out2_2560to1280_up     3.10e-3 / 3.82e-3                         out3_2560to1280_xf     5.05e-3 / 4.51e-3, 6.69e-3 / 6.81e-3
    out5_1920to1280_xf_up  5.49e-3 / 6.29e-3                         out6_1920to640_xf      5.08e-3 / 5.85e-3, 6.90e-3 / 8.67e-3
    out7_1280to640_xf      5.18e-3 / 5.08e-3, 7.06e-3 / 7.02e-3      out8_960to640_xf_up    5.46e-3 / 5.67e-3
    out9_960to320_xf       5.13e-3 / 6.25e-3, 6.84e-3 / 7.81e-3      out10_640to320_xf      5.19e-3 / 7.10e-3, 7.12e-3 / 1.01e-2
    product_320_64x64      4.00e-3 / 4.87e-3, 5.58e-3 / 6.40e-3      product_640_32x32      4.37e-3 / 5.14e-3, 5.91e-3 / 7.28e-3
    product_1280_16x16     4.56e-3 / 5.47e-3, 6.16e-3 / 7.42e-3      ragged_320             4.61e-3 / 6.08e-3, 6.32e-3 / 7.86e-3
    ragged_640             5.09e-3 / 5.95e-3, 6.93e-3 / 8.27e-3      ragged_1280            4.95e-3 / 6.18e-3, 6.71e-3 / 7.25e-3
    ragged_up              5.12e-3 / 5.03e-3                         ragged_down            1.67e-3 / 2.44e-3
    batch_xf               4.86e-3 / 5.87e-3, 6.44e-3 / 8.68e-3      batch_up               5.36e-3 / 5.75e-3

batch_up found a bug, fixed with it: item 1 of the batch of two through output_blocks.5 (1920 -> 1280 + transformer + Upsample) differed from
that item run alone in 90 of 327 680 elements by one bf16 step (rel-L2 1.22e-5). ir_igemm_splitk() took the split count from the whole launch's
tile count (the up-conv: 20 tiles and 12 splits at M = 256, 40 tiles and 6 splits at M = 512); it now takes it from one item's tiles. See
docs/parity.md.
"""
import time

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import unet_block_ref as R

pytestmark = pytest.mark.gpu

FAST_OVER_PLAIN = 1.15
CANARY = 0x5A5B   # bf16 bits of the canary columns and the tail behind `out`
GUARD_COLS, TAIL = 64, 4096
K_CONV_GENERIC, K_GN, K_TRANSPOSE, K_FLASH, K_OTHER = ("conv3x3/igemm_kernel<taps=9>", "groupnorm/gn_partial+gn_finalize+gn_apply", "transpose/transpose_v*",
                                                       "flash_attn/other", "other/layout+glue")
# case -> launches of (the generic 3x3 kernel = the split-K route of the convs: K split over extra workgroups where a launch has at most 48
# output tiles and at least 24 k-tiles of 64, which at these pixel counts is every 3x3 conv of 64-multiple width but those of the 64 x 64 case;
# groupnorm_any: two per ResBlock, one per transformer; transpose_v; the flash kernel of the self- and the cross-attention; geglu)
ROUTES = {
    "in0_conv": (1, 0, 0, 0, 0),   # (the generic kernel without a split: 32 input channels are no multiple of a 64-wide k-tile)
    "in1_xf320": (2, 3, 1, 2, 1),
    "in4_320to640_xf": (2, 3, 1, 2, 1),
    "in5_xf640": (2, 3, 1, 2, 1),
    "in7_640to1280_xf": (2, 3, 1, 2, 1),
    "in8_xf1280": (2, 3, 1, 2, 1),
    "in10_res1280": (2, 2, 0, 0, 0),
    "in3_down320": (1, 0, 0, 0, 0),
    "in6_down640": (1, 0, 0, 0, 0),
    "in9_down1280": (1, 0, 0, 0, 0),
    "mid0_res": (2, 2, 0, 0, 0),
    "mid1_xf": (0, 1, 1, 2, 1),
    "mid2_res": (2, 2, 0, 0, 0),
    "out0_2560to1280": (2, 2, 0, 0, 0),
    "out2_2560to1280_up": (3, 2, 0, 0, 0),
    "out3_2560to1280_xf": (2, 3, 1, 2, 1),
    "out5_1920to1280_xf_up": (3, 3, 1, 2, 1),
    "out6_1920to640_xf": (2, 3, 1, 2, 1),
    "out7_1280to640_xf": (2, 3, 1, 2, 1),
    "out8_960to640_xf_up": (3, 3, 1, 2, 1),
    "out9_960to320_xf": (2, 3, 1, 2, 1),
    "out10_640to320_xf": (2, 3, 1, 2, 1),
    "product_320_64x64": (0, 3, 1, 2, 1),
    "product_640_32x32": (2, 3, 1, 2, 1),
    "product_1280_16x16": (2, 3, 1, 2, 1),
    "ragged_320": (2, 3, 1, 2, 1),
    "ragged_640": (2, 3, 1, 2, 1),
    "ragged_1280": (2, 3, 1, 2, 1),
    "ragged_up": (3, 3, 1, 2, 1),
    "ragged_down": (1, 0, 0, 0, 0),
    "batch_xf": (2, 3, 1, 2, 1),
    "batch_up": (3, 3, 1, 2, 1),
}
UNET_PARAMS = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
                   num_head_channels=64, use_spatial_transformer=True, use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, legacy=False)


@pytest.fixture(scope="module")
def net():
    """(UNetWeights, the uploaded ControlledUnetModel, the context [1][77][1024]) - one full-width UNet for the module."""
    from instarevive_amd.cldm import ControlledUnetModel
    t0 = time.time()
    W = R.UNetWeights()
    sd = W.full_sd()
    t1 = time.time()
    m = ControlledUnetModel(**UNET_PARAMS)
    m.load_state_dict(sd, strict=True)
    # a context of the module's own: the shared one may hold another module's ControlNet, whose context width ir_unet_set_context checks
    m.ctx = L.Context(0)
    m.device = m.ctx.device
    m._upload()
    torch.cuda.synchronize()
    print(f"\nfull-width UNet: weights {t1 - t0:.1f} s, pack + upload {time.time() - t1:.1f} s")
    yield W, m, R.make_context(W).float()[None].contiguous()
    m.ctx = None


@pytest.fixture(autouse=True)
def exact_reference():
    """No TF32 / reduced-precision products inside the reference."""
    mm, cd = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = mm, cd


def bind(m, ctxt):
    from instarevive_amd.cldm import _set_context
    m._ready()
    _set_context(m.ctx, ctxt)


def device_rows(x, cin_dev):
    """bf16 device rows of x (float64 holding bf16 values), zero-padded to cin_dev columns (input_blocks.0 reads 32)."""
    xd = torch.zeros(x.shape[0], cin_dev, dtype=torch.bfloat16, device="cuda")
    xd[:, :x.shape[1]] = x.to(torch.bfloat16)
    return xd


def out_rows(n, h, w, scale):
    return n * h * w * 4 if scale == 2 else n * (h // 2) * (w // 2) if scale == -2 else n * h * w


def launch(ctx, set_, index, xd, n, h, w, cout, rows, short=0, out_cs=None, which=0):
    """ir_op_unet_block into a canary-filled buffer with a workspace of exactly ir_op_unet_block_ws bytes (less `short`) of 0xFF: returns
    (return code, the block's columns [rows][cout] as a copy). Checks the canary columns and tail, and that a refused call wrote nothing."""
    cs = cout + GUARD_COLS if out_cs is None else out_cs
    need = int(ctx.lib.ir_op_unet_block_ws(ctx.h, which, set_, index, n, h, w)) or 4096   # (0: the query refuses these arguments, and so must the call)
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    buf = torch.full((rows * max(cs, cout) + TAIL,), CANARY, dtype=torch.int16, device="cuda")
    rc = ctx.lib.ir_op_unet_block(ctx.h, ctx.stream(), which, set_, index, L.ptr(xd), L.ptr(buf), cs, n, h, w, R.TIMESTEP, L.ptr(ws), need - short)
    torch.cuda.synchronize()
    if rc != 0:
        assert bool((buf == CANARY).all()), f"a refused call (rc {rc}) wrote to the output"
        return rc, None
    body = buf[:rows * cs].view(rows, cs)
    assert bool((body[:, cout:] == CANARY).all()), "the block wrote outside its column slice"
    assert bool((buf[rows * cs:] == CANARY).all()), "the block wrote behind its output"
    return rc, body[:, :cout].contiguous().view(torch.bfloat16)


def run(ctx, case, xd, what, n=None):
    set_, index, n0, h, w = R.CASES[case]
    n = n0 if n is None else n
    cin, cout, kind, scale = R.block_io(R.CFG, set_, index)
    rc, out = launch(ctx, set_, index, xd, n, h, w, cout, out_rows(n, h, w, scale))
    ctx.check(rc, what)
    assert torch.isfinite(out.float()).all(), f"{what}: an output element is not finite"
    return out


@torch.no_grad()
def reference(W, case, ctxt):
    """(x, reference rows, emulation rows, update base) of a case, float64 on the CPU, computed on the GPU."""
    set_, index, n, h, w = R.CASES[case]
    x = R.case_inputs(W, case)[0]
    xd, cd = x.cuda(), ctxt[0].double().cuda()
    ref, base = R.block(W, set_, index, xd, n, h, w, R.time_emb(W, R.TIMESTEP, "cuda"), cd)
    emu, _ = R.block(W, set_, index, xd, n, h, w, R.time_emb(W, R.TIMESTEP, "cuda", emulate=True), cd, emulate=True)
    base = R.update_base(W, set_, index, xd, base)
    out = x, ref.cpu(), emu.cpu(), None if base is None else base.cpu()
    W.drop_device_copies()
    torch.cuda.empty_cache()
    return out


def gate(what, got, ref, base, kind):
    e = R.errors(got.cpu(), ref, base)
    print(f"GATE {what}: " + " ".join("   -    " if v is None else f"{v:.2e}" for v in e))
    assert R.inside(e, R.GATES[kind]), f"{what}: {e} against the gates {R.GATES[kind]}"
    return e[0]


@pytest.mark.parametrize("case", list(R.CASES))
def test_unet_block(net, case):
    W, m, ctxt = net
    bind(m, ctxt)
    ctx = m.ctx
    set_, index, n, h, w = R.CASES[case]
    cin, cout, kind, scale = R.block_io(R.CFG, set_, index)
    what = f"unet_block {case} (set {set_} block {index}, {kind}, n {n}, {h} x {w})"
    x, ref, emu, base = reference(W, case, ctxt)
    e = R.errors(emu, ref, base)
    print(f"\nEMULATION {what}: " + " ".join("   -    " if v is None else f"{v:.2e}" for v in e))
    assert R.inside(e, tuple(None if g is None else g / 2 for g in R.GATES[kind])), f"{what}: the bf16 emulation {e} is not under half of the gates {R.GATES[kind]}"
    xd = device_rows(x, 32 if kind == "conv0" else cin)
    a = run(ctx, case, xd, what)
    ctx.profile_begin()
    b = run(ctx, case, xd, what + " again")
    rows = ctx.profile_end_kernels()
    print(f"{what}: launches " + ", ".join(f"{k} x{v['launches']}" for k, v in sorted(rows.items())))
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: two launches differ"
    l2_fast = gate(what, a, ref, base, kind)
    try:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        c = run(ctx, case, xd, what + " plain")
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
    l2_plain = gate(what + " plain", c, ref, base, kind)
    print(f"RATIO {what}: fast / plain rel-L2 {l2_fast / l2_plain:.3f}")
    assert l2_fast <= FAST_OVER_PLAIN * l2_plain, f"{what}: fast route rel-L2 {l2_fast:.3e} against the plain route's {l2_plain:.3e}"
    if n > 1:   # item 1 alone
        Ti, To = h * w, out_rows(1, h, w, scale)
        solo = run(ctx, case, xd[Ti:2 * Ti].contiguous(), what + " item 1 alone", n=1)
        d = a[To:2 * To].double() - solo.double()
        print(f"BATCH {what}: item 1 of the batch against item 1 alone: {int((d != 0).sum())} of {d.numel()} elements differ, rel-L2 {float(d.norm() / solo.double().norm()):.2e}, "
              f"worst {float(d.abs().max() / solo.double().abs().max()):.2e} of max |out|; alone: " + " ".join(
                  "   -    " if v is None else f"{v:.2e}" for v in R.errors(solo.cpu(), ref[To:2 * To], None if base is None else base[Ti:2 * Ti])))
        assert torch.equal(a[To:2 * To].view(torch.int16), solo.view(torch.int16)), f"{what}: item 1 of the batch differs from item 1 run alone"
    for k, cnt in zip((K_CONV_GENERIC, K_GN, K_TRANSPOSE, K_FLASH, K_OTHER), ROUTES[case]):
        got = rows.get(k, {}).get("launches", 0)
        assert got == cnt, f"{what}: {k} launched {got} times, expected {cnt}"


def test_unet_block_refuses_bad_arguments(net):
    """-1 for a UNet, set or index that is not there, -10 for non-positive sizes, -1 for out_cs < cout, a missing tensor and an odd grid on a
    Downsample, -20 for a workspace one byte short (nothing written), -11 for a transformer block of a UNet whose context was never set -
    whose ResBlock-only blocks run; the workspace query answers every refused argument set with 0."""
    W, m, ctxt = net
    bind(m, ctxt)
    ctx = m.ctx
    lib = ctx.lib
    xd = torch.zeros(2 * 64, 2560, dtype=torch.bfloat16, device="cuda")

    def rc(set_, index, n=1, h=8, w=8, which=0, cout=1280, **kw):
        return launch(ctx, set_, index, xd, n, h, w, cout, 4 * max(n, 1) * 64, which=which, **kw)[0]

    assert rc(0, 8) == 0 and rc(2, 2) == 0
    for which, set_, index in ((2, 0, 1), (-1, 0, 1), (0, 3, 0), (0, -1, 0), (0, 0, 12), (0, 1, 3), (0, 2, 12), (0, 0, -1)):
        assert lib.ir_op_unet_block_ws(ctx.h, which, set_, index, 1, 8, 8) == 0
        assert rc(set_, index, which=which) == -1, (which, set_, index)
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, -8), (-1, 8, 8)):
        assert lib.ir_op_unet_block_ws(ctx.h, 0, 0, 8, n, h, w) == 0
        assert rc(0, 8, n=n, h=h, w=w) == -10, (n, h, w)
    assert rc(0, 8, out_cs=1272) == -1 and rc(0, 8, out_cs=0) == -1
    assert rc(0, 9, h=7) == -1 and rc(0, 9, w=9) == -1 and lib.ir_op_unet_block_ws(ctx.h, 0, 0, 9, 1, 7, 8) == 0
    assert rc(0, 9, h=6, w=10) == 0
    assert rc(0, 8, short=1) == -20 and rc(2, 2, short=1) == -20
    need = int(lib.ir_op_unet_block_ws(ctx.h, 0, 0, 8, 1, 8, 8))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros(64, 1280, dtype=torch.bfloat16, device="cuda")
    assert lib.ir_op_unet_block(ctx.h, ctx.stream(), 0, 0, 8, None, L.ptr(out), 1280, 1, 8, 8, R.TIMESTEP, L.ptr(ws), need) == -1
    assert lib.ir_op_unet_block(ctx.h, ctx.stream(), 0, 0, 8, L.ptr(xd), None, 1280, 1, 8, 8, R.TIMESTEP, L.ptr(ws), need) == -1
    assert lib.ir_op_unet_block(ctx.h, ctx.stream(), 0, 0, 8, L.ptr(xd), L.ptr(out), 1280, 1, 8, 8, R.TIMESTEP, None, need) == -20
    # a context without a UNet, then with a (small) UNet whose context was never set
    from instarevive_amd.cldm import ControlledUnetModel
    from tests.golden._det import det_state_dict
    from oracle import cldm as ocldm
    bare = L.Context(0)
    assert bare.lib.ir_op_unet_block(bare.h, bare.stream(), 0, 0, 1, L.ptr(xd), L.ptr(out), 1280, 1, 8, 8, R.TIMESTEP, L.ptr(ws), need) == -1
    assert bare.lib.ir_op_unet_block_ws(bare.h, 0, 0, 1, 1, 8, 8) == 0
    small = ControlledUnetModel(**dict(UNET_PARAMS, model_channels=64, num_head_channels=32, context_dim=64))
    small.load_state_dict(det_state_dict(ocldm.state_dict_shapes(R.CLDM_SMALL), seed=707))
    small.ctx, small.device = bare, bare.device
    small._upload()
    assert launch(bare, 0, 8, xd, 1, 8, 8, 256, 64)[0] == -11 and bare.lib.ir_op_unet_block_ws(bare.h, 0, 0, 8, 1, 8, 8) == 0
    assert launch(bare, 0, 10, xd, 1, 8, 8, 256, 64)[0] == 0
    assert lib.ir_op_unet_block(None, None, 0, 0, 0, None, None, 0, 1, 8, 8, R.TIMESTEP, None, 0) == -11
