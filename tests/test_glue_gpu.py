"""The glue between the networks and the picture, called through the C ABI on its own: ir_color_fix (wavelet_level / add2 / plane_stats /
adain_apply kernels), ir_tiled_count, ir_tiled_blend_latent and ir_tiled_blend_pixels (zero_f32 / tile_add / tile_div with window_count() /
nchw_to_u8 kernels) against the float64 references of tests/support/glue_ref.py. No model, no weights.

Gates (derived in tests/test_glue_ref_cpu.py from the reference's own precision, never from the HIP result):
  wavelet  max-abs error <= 4 x the max-abs error of the float32 oracle.glue.wavelet_reconstruction against the float64 reference on the
           case's inputs (no summation order is pinned); at 32x512x512 on four of the 32 items, which can only narrow the gate
           (glue_ref.product_wavelet_gate)
  AdaIN    max-abs error <= 4 x the max-abs error of float64 statistics rounded to float32 and applied in float32 (adain_apply32)
  blends   the float32 result has the bits of blend32 (adds in loop order from a zero buffer, one IEEE division by the count): the tile-sharded
           multi-GPU run's "single-GPU result bit for bit" rests on that order; the bytes are to_u8(blend32), and against the float64 blend
           they differ by at most 1 and only where the float64 value * 255 lies within 1e-3 of an integer (at most 0.5 % of a frame)
Every blend also runs on poison-filled outputs twice (two poisons: nothing skipped, the same bits again), and in a second pass on tiles cropped
from one frame, which must come back exactly where the overlap count is 1, 2 or 4, within 1 ulp at counts 3 and 6 and within 2 ulp at count 9,
where the fp32 loop in loop order is itself 2 ulp off (tests/test_glue_ref_cpu.py). Every call passes exactly the workspace size the library
reports as needed, not the size of the context's grow-only buffer.

Measured on the MI355X: max-abs error against the float64 reference (share of the case's gate).
    case          wavelet              AdaIN
    2x2           8.64e-08 (0.25)      6.41e-07 (0.25)
    8x24          1.69e-07 (0.25)      2.82e-07 (0.25)
    24x8_n3       1.85e-07 (0.25)      3.49e-07 (0.25)
    16x16         1.54e-07 (0.25)      5.71e-07 (0.25)
    64x64_n2      2.56e-07 (0.25)      4.82e-07 (0.25)
    72x200        2.54e-07 (0.25)      1.26e-07 (0.21)
    64x64_n33     2.83e-07 (0.25)      1.55e-07 (0.23)
    mean100             -              9.36e-06 (0.25)
    const_style         -              3.94e-07 (0.25)
    const_content       -              3.94e-07 (0.25)
    32x512x512    3.42e-07 (0.27)      1.23e-06 (0.25)
    cf_fixture    1.59e-07 (0.25)      8.61e-08 (0.23)
    drop-in wrappers (every case above; plain, non-contiguous and float16 arguments, 32x512x512 and cf_fixture plain): 0.19 .. 0.36 of the gate
    mean100: the gate is 3.74e-07 of the output's magnitude (100)
    against the reference's recorded float32 outputs: wavelet 0.000e+00, adain 5.960e-08
Blends: all 14 latent geometries bit-equal to blend32 (no difference seen, so no ulp gate is used); against the float64 blend 0.0e+00 .. 1.1e-07.
Bytes: equal to to_u8(blend32) in all 14 geometries; against the float64 bytes 10 of 12214272 differ (most: 6, of 10027008), each by 1 and at a byte boundary; 0.188 .. 0.216 % of a frame lies at one (allowed 0.5 %).
Cropped tiles: 0 ulp at counts 1, 2, 4 in every geometry, 1.00 ulp at counts 3 and 6 (tile_is_height, depth3, depth3x3, small_40_n1, small_40_n2, small_40_n3), 1.00 ulp at count 9 (depth3x3, allowed 2).
The file: 79 tests in 5.19 s on the MI355X; the slowest is the 32x512x512 wavelet case (float64 reference on the GPU, float32 oracle on the host), 1.03 s.
"""
import os

import numpy as np
import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import glue_ref as R

pytestmark = pytest.mark.gpu

KINDS = {"wavelet": (L.FLAG_FIX_WAVELET, R.wavelet_fix64, R.wavelet_gate), "adain": (L.FLAG_FIX_ADAIN, R.adain_fix64, R.adain_gate)}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUNDARY_SHARE = 0.005


def _last_error(ctx):
    msg = ctx.lib.ir_last_error(ctx.h)
    return msg.decode() if msg else ""


def _color_fix_rc(ctx, kind, c, s, out, ws, ws_bytes):
    n, _, h, w = c.shape
    rc = ctx.lib.ir_color_fix(ctx.h, ctx.stream(), kind, L.ptr(c), L.ptr(s), L.ptr(out), n, h, w, L.ptr(ws), ws_bytes)
    torch.cuda.synchronize()
    return rc


def color_fix(ctx, kind, c, s):
    """ir_color_fix on device tensors into a NaN-filled output, with exactly the workspace ir_workspace_bytes(IR_STAGE_COLORFIX) reports (the
    context's buffer only grows, so its own size would say nothing about this case's need)."""
    n, _, h, w = c.shape
    out = torch.full_like(c, float("nan"))
    need = ctx.ws_bytes(L.STAGE_COLORFIX, n, h, w)
    ws = ctx.workspace(need)
    ctx.check(_color_fix_rc(ctx, kind, c, s, out, ws, need), "ir_color_fix")
    return out


def _report(what, err, gate):
    print(f"GLUE {what}: max-abs error {err:.3e}, gate {gate:.3e}, {err / gate:.2f} of the gate")


def _check_fix(ctx, name, kind, c, s, want, gate):
    got = color_fix(ctx, KINDS[kind][0], c, s)
    assert not bool(torch.isnan(got).any()), f"{name}: output elements left unwritten"
    err = float((got.double() - want.to(got.device)).abs().max())
    _report(f"{kind} {name}", err, gate)
    assert err <= gate, (name, kind, err, gate)
    return got


def _colorfix_case(name, kind):
    if name in R.ADAIN_SPECIAL:
        return R.adain_special_inputs(name)
    return R.colorfix_inputs(*R.COLORFIX_CASES[name])


CF_PARAMS = [(k, "wavelet") for k in R.COLORFIX_CASES] + [(k, "adain") for k in R.COLORFIX_CASES] + [(k, "adain") for k in R.ADAIN_SPECIAL]


# ------------------------------------------------------------------------------------------------ ir_color_fix
@pytest.mark.parametrize("name,kind", CF_PARAMS)
def test_color_fix(ctx, name, kind):
    c, s = _colorfix_case(name, kind)
    _, ref, gate = KINDS[kind]
    want = ref(c, s)
    got = _check_fix(ctx, name, kind, c.cuda(), s.cuda(), want, gate(c, s))
    if name == "mean100":
        print(f"GLUE adain mean100: gate relative to the output's magnitude {gate(c, s) / float(want.abs().max()):.2e}")
    if name == "const_content":   # a constant content plane becomes the style's mean
        assert float((got[0, 1].double().cpu() - s[0, 1].double().mean()).abs().max()) <= 1e-7


@pytest.fixture(scope="module")
def product():
    """32 x 3 x 512 x 512: the launch decode_tiles_run makes at tile 512 (TILE_BATCH tiles). Inputs on the GPU, the float64 references computed
    there, once for the direct and the wrapper test. The AdaIN yardstick is taken on all 32 items, the wavelet yardstick (float32 oracle on the
    host) on four of them, which can only narrow the gate: see glue_ref.product_wavelet_gate."""
    c, s = R.product_inputs("cuda")
    return c, s, {"wavelet": (R.wavelet_fix64(c, s), R.product_wavelet_gate(c, s)), "adain": (R.adain_fix64(c, s), R.adain_gate(c, s))}


@pytest.mark.parametrize("kind", ["wavelet", "adain"])
def test_color_fix_product_launch(ctx, product, kind):
    c, s, refs = product
    _check_fix(ctx, "32x512x512", kind, c, s, *refs[kind])


def _fixture_case():
    fx = np.load(os.path.join(GOLD, "glue.npz"))
    return fx, torch.from_numpy(fx["cf_content"]), torch.from_numpy(fx["cf_style"])


@pytest.mark.parametrize("kind", ["wavelet", "adain"])
def test_color_fix_reference_fixture(ctx, kind):
    """The reference's own recorded colour-fix outputs (float32, so they sit one yardstick away from the float64 reference themselves)."""
    fx, c, s = _fixture_case()
    _, ref, gate = KINDS[kind]
    got = _check_fix(ctx, "cf_fixture", kind, c.cuda(), s.cuda(), ref(c, s), gate(c, s))
    rec = torch.from_numpy(fx["cf_" + kind])
    err = float((got.cpu().double() - rec.double()).abs().max())
    print(f"GLUE {kind} against the reference's recorded float32 output: {err:.3e}")
    assert err <= 2e-6


def _wrapper(kind):
    from instarevive_amd import pipeline as P
    return {"wavelet": P.wavelet_reconstruction, "adain": P.adaptive_instance_normalization}[kind]


def _check_wrapper(kind, what, cd, sd, want=None, g=None):
    """The drop-in wrapper on device tensors of any layout and float type: float32 out, judged on the values the wrapper was given."""
    _, ref, gate = KINDS[kind]
    got = _wrapper(kind)(cd, sd)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == cd.shape and got.is_contiguous()
    if want is None:
        c32, s32 = cd.float().cpu().contiguous(), sd.float().cpu().contiguous()
        want, g = ref(c32, s32), gate(c32, s32)
    err = float((got.double() - want.to(got.device)).abs().max())
    _report(f"{kind} wrapper {what}", err, g)
    assert err <= g, (what, err, g)


@pytest.mark.parametrize("name,kind", CF_PARAMS)
def test_color_fix_drop_in_wrappers(ctx, name, kind):
    """pipeline.wavelet_reconstruction / adaptive_instance_normalization on every case of test_color_fix, each with plain, non-contiguous and
    float16 arguments (the float16 values are the case's inputs rounded: reference and gate are taken on what the wrapper receives)."""
    c, s = _colorfix_case(name, kind)
    forms = {"plain": (c.cuda(), s.cuda()),
             "non-contiguous": (c.transpose(2, 3).contiguous().cuda().transpose(2, 3), s.transpose(2, 3).contiguous().cuda().transpose(2, 3)),
             "float16": (c.half().cuda(), s.half().cuda())}
    assert not forms["non-contiguous"][0].is_contiguous() and torch.equal(forms["non-contiguous"][0].cpu(), c)
    for form, (cd, sd) in forms.items():
        _check_wrapper(kind, f"{name} {form}", cd, sd)


@pytest.mark.parametrize("kind", ["wavelet", "adain"])
def test_color_fix_drop_in_wrappers_product_launch_and_fixture(ctx, product, kind):
    """The two large or recorded cases through the wrappers, in plain form."""
    c, s, refs = product
    _check_wrapper(kind, "32x512x512 plain", c, s, *refs[kind])
    _, fc, fs = _fixture_case()
    _check_wrapper(kind, "cf_fixture plain", fc.cuda(), fs.cuda())


def test_color_fix_refusals(ctx):
    n, h, w = 2, 24, 40
    c, s = (t.cuda() for t in R.colorfix_inputs(n, h, w))
    out = torch.full_like(c, float("nan"))
    need = (3 * n * 3 * h * w * 4 + 255) // 256 * 256      # wavelet: ping, pong and the high band
    ws = ctx.workspace(need + 4096)
    assert _color_fix_rc(ctx, L.FLAG_FIX_WAVELET, c, s, out, ws, need) == 0
    assert not bool(torch.isnan(out).any())
    out.fill_(float("nan"))
    assert _color_fix_rc(ctx, L.FLAG_FIX_WAVELET, c, s, out, ws, need - 4) == -20      # one float short
    msg = _last_error(ctx)
    assert "workspace too small" in msg and str(need) in msg and str(need - 4) in msg, msg
    assert bool(torch.isnan(out).all())                                                  # nothing was launched
    for kind in (0, L.FLAG_FIX_WAVELET | L.FLAG_FIX_ADAIN, L.FLAG_TILED):
        assert _color_fix_rc(ctx, kind, c, s, out, ws, need) == -11
        assert "bad colour-fix kind" in _last_error(ctx)
    one = torch.zeros(1, 3, 1, 1, device="cuda")                                         # no unbiased variance of one sample
    o1 = torch.full_like(one, float("nan"))
    assert _color_fix_rc(ctx, L.FLAG_FIX_ADAIN, one, one, o1, ws, need) != 0
    assert "adain_fix" in _last_error(ctx) and bool(torch.isnan(o1).all())
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ tile blends
POISON_F32 = (float("nan"), 12345.0)
POISON_U8 = (0xA5, 0x5A)


def _pixel_ws_bytes(n, h, w):
    """ir_tiled_blend_pixels allocates the float32 frame and nothing else: sized directly, to the byte (the arena rounds to 256), so that no model
    has to be configured (the header's ir_workspace_bytes(IR_STAGE_PIPELINE, ... | IR_FLAG_TILED) is the whole pipeline's need, which contains
    this). test_blend_pixels_workspace_one_float_short shows that nothing less is accepted."""
    return (n * 3 * h * w * 4 + 255) // 256 * 256


def blend_latent_rc(ctx, tiles, out, n, h, w, tile, stride):
    rc = ctx.lib.ir_tiled_blend_latent(ctx.h, ctx.stream(), L.ptr(tiles), L.ptr(out), n, h, w, tile, stride)
    torch.cuda.synchronize()
    return rc


def blend_pixels_rc(ctx, tiles, out, n, h, w, tile, stride, short=0):
    need = _pixel_ws_bytes(n, h, w)
    ws = ctx.workspace(need)
    rc = ctx.lib.ir_tiled_blend_pixels(ctx.h, ctx.stream(), L.ptr(tiles), L.ptr(out), n, h, w, tile, stride, L.ptr(ws), need - short)
    torch.cuda.synchronize()
    return rc


def blend_latent(ctx, tiles, n, h, w, tile, stride):
    """ir_tiled_blend_latent (sizes in pixels) on host tiles [K][n][4][t/8][t/8], twice on differently poisoned outputs."""
    K = len(R.windows(h // 8, w // 8, tile // 8, stride // 8))
    assert tuple(tiles.shape) == (K, n, 4, tile // 8, tile // 8) and ctx.lib.ir_tiled_count(h, w, tile, stride) == K
    td, outs = tiles.contiguous().cuda(), []
    for poison in POISON_F32:
        out = torch.full((n, 4, h // 8, w // 8), poison, dtype=torch.float32, device="cuda")
        ctx.check(blend_latent_rc(ctx, td, out, n, h, w, tile, stride), "ir_tiled_blend_latent")
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "poison shows through, or a second call gives other bits"
    return outs[0]


def blend_pixels(ctx, tiles, n, h, w, tile, stride):
    K = len(R.windows(h, w, tile, stride))
    assert tuple(tiles.shape) == (K, n, 3, tile, tile) and ctx.lib.ir_tiled_count(h, w, tile, stride) == K
    td, outs = tiles.contiguous().cuda(), []
    for poison in POISON_U8:
        out = torch.full((n, h, w, 3), poison, dtype=torch.uint8, device="cuda")
        ctx.check(blend_pixels_rc(ctx, td, out, n, h, w, tile, stride), "ir_tiled_blend_pixels")
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), "poison shows through, or a second call gives other bits"
    return outs[0]


def _ulps(got, want):
    return float(((got.double() - want.double()).abs() / R.ulp32(want)).max())


@pytest.mark.parametrize("case", list(R.BLEND_CASES))
def test_blend_latent_has_the_bits_of_the_loop_order_sum(ctx, case):
    n, h, w, tile, stride = R.BLEND_CASES[case]
    tiles, geo = R.blend_tiles(case, 4)
    got = blend_latent(ctx, tiles, n, h, w, tile, stride)
    want = R.blend32(tiles, *geo)
    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
    e64 = float((got.double() - R.blend64(tiles, *geo)).abs().max())
    print(f"GLUE blend_latent {case}: {len(tiles)} tiles, bit-equal to blend32: {same}"
          f"{'' if same else f' (max {_ulps(got, want):.2f} ulp)'}, against float64 {e64:.3e}")
    assert same


@pytest.mark.parametrize("case", list(R.BLEND_CASES))
def test_blend_pixels_bytes(ctx, case):
    n, h, w, tile, stride = R.BLEND_CASES[case]
    tiles, geo = R.blend_tiles(case, 3)
    got = blend_pixels(ctx, tiles, n, h, w, tile, stride)
    b64 = R.blend64(tiles, *geo)
    assert torch.equal(got, R.to_u8(R.blend32(tiles, *geo)))
    u64, near = R.to_u8(b64), R.u8_boundary(b64)
    diff = got != u64
    share = float(near.double().mean())
    print(f"GLUE blend_pixels {case}: {len(tiles)} tiles, bytes equal to_u8(blend32); against float64 bytes {int(diff.sum())} of {diff.numel()} differ, "
          f"all at a byte boundary ({100 * share:.3f} % of the frame lies at one)")
    assert share <= BOUNDARY_SHARE
    assert not bool((diff & ~near).any()) and int((got.int() - u64.int()).abs().max()) <= 1


@pytest.mark.parametrize("case", list(R.CROP_CASES))
def test_cropped_tiles_blend_back_to_their_frame(ctx, case):
    n, h, w, tile, stride = R.BLEND_CASES[case]
    lh, lw, tl, sl = h // 8, w // 8, tile // 8, stride // 8
    frame = R.image(n, lh, lw, 9, 4)
    got = blend_latent(ctx, R.crop_tiles(frame, tl, sl), n, h, w, tile, stride)
    cnt = R.counts(lh, lw, tl, sl).expand_as(frame)
    pow2 = (cnt == 1) | (cnt == 2) | (cnt == 4)
    assert torch.equal(got[pow2], frame[pow2])
    worst = {k: _ulps(got[cnt == k], frame[cnt == k]) for k in sorted(set(cnt.flatten().tolist()))}
    print(f"GLUE crop pass {case}: worst ulp per count {worst}")
    for k, e in worst.items():        # exact at 1, 2, 4; 1 ulp at 3 and 6; 2 ulp at 9, where the fp32 loop itself is 2 ulp off (glue_ref.CROP_ULP)
        assert e <= R.CROP_ULP[k], (case, k, e)
    pf = R.image(n, h, w, 11)
    gb = blend_pixels(ctx, R.crop_tiles(pf, tile, stride), n, h, w, tile, stride)
    want, near = R.to_u8(pf), R.u8_boundary(pf)
    pcnt = R.counts(h, w, tile, stride)[None, :, :, None].expand_as(want)
    exact = (pcnt == 1) | (pcnt == 2) | (pcnt == 4)
    assert torch.equal(gb[exact], want[exact])
    assert not bool(((gb != want) & ~near).any()) and int((gb.int() - want.int()).abs().max()) <= 1


@pytest.mark.parametrize("case", ["small_40_n2", "depth3x3", "ragged_y"])
def test_blend_pixels_truncates_and_clamps(ctx, case):
    n, h, w, tile, stride = R.BLEND_CASES[case]
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    k = torch.stack([torch.stack([(yy * 7 + xx * 3 + c * 11 + i * 5) % 256 for c in range(3)], 0) for i in range(n)], 0)
    frame = ((k.double() + 0.5) / 255).float()                        # every value half a byte above a boundary
    got = blend_pixels(ctx, R.crop_tiles(frame, tile, stride), n, h, w, tile, stride)
    assert torch.equal(got, k.permute(0, 2, 3, 1).to(torch.uint8))
    assert set(R.counts(h, w, tile, stride).flatten().tolist()) > {1, 2}
    values = torch.tensor([-0.25, 0.0, 1.0, 1.5, 0.5, -1e-3, 1.0 + 1e-3, 254.5 / 255])
    want = torch.tensor([0, 0, 255, 255, 127, 0, 255, 254], dtype=torch.uint8)
    idx = (yy * 5 + xx) % len(values)
    idx = torch.stack([torch.stack([(idx + c + 2 * i) % len(values) for c in range(3)], 0) for i in range(n)], 0)
    got = blend_pixels(ctx, R.crop_tiles(values[idx], tile, stride), n, h, w, tile, stride)
    assert torch.equal(got, want[idx].permute(0, 2, 3, 1))


def test_tiled_count_equals_the_window_list(ctx):
    for h, w, t, s in R.count_sweep():
        assert ctx.lib.ir_tiled_count(h, w, t, s) == len(R.windows(h // 8, w // 8, t // 8, s // 8)), (h, w, t, s)
    assert ctx.lib.ir_tiled_count(2176, 3840, 512, 448) == 45


@pytest.mark.parametrize("why", list(R.BAD_GEOMETRIES))
def test_bad_tile_geometry_is_refused(ctx, why):
    """-31 with "bad tile geometry" and an untouched output. stride > tile used to be accepted: the windows then leave pixels uncovered,
    tile_div divided 0 by 0 there and the bytes came out as black stripes."""
    h, w, tile, stride = R.BAD_GEOMETRIES[why]
    n = 1
    assert ctx.lib.ir_tiled_count(h, w, tile, stride) == -31
    K = max(1, len(R.windows(h // 8, w // 8, max(tile // 8, 1), max(stride // 8, 1))))     # room for every tile the geometry would name
    lat = torch.ones((K, n, 4, tile // 8, tile // 8), device="cuda")
    nb = torch.full((n, 4, h // 8, w // 8), 7.0, device="cuda")
    assert blend_latent_rc(ctx, lat, nb, n, h, w, tile, stride) == -31
    assert "bad tile geometry" in _last_error(ctx)
    assert bool((nb == 7.0).all())
    tp = tile // 8 * 8
    px = torch.ones((K, n, 3, tp, tp), device="cuda")
    out = torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    assert blend_pixels_rc(ctx, px, out, n, h, w, tile, stride) == -31
    assert "bad tile geometry" in _last_error(ctx)
    assert bool((out == 0xA5).all())


def test_blend_pixels_workspace_one_float_short(ctx):
    n, h, w, tile, stride = R.BLEND_CASES["ragged_y"]
    tiles = R.blend_tiles("ragged_y", 3)[0].cuda()
    out = torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    assert blend_pixels_rc(ctx, tiles, out, n, h, w, tile, stride, short=4) == -20
    msg = _last_error(ctx)
    need = _pixel_ws_bytes(n, h, w)
    assert "workspace too small" in msg and str(need) in msg and str(need - 4) in msg, msg
    assert bool((out == 0xA5).all())                                                       # nothing was launched


class _NeverCalled:
    def __call__(self, *a, **k):
        raise AssertionError("a network ran before the tile geometry was checked")


@pytest.mark.parametrize("fused", [True, False])
def test_process_refuses_stride_above_tile(ctx, fused):
    """The whole path (fused ir_pipeline and the stage-by-stage form) raises instead of returning a picture; so does HipTileEngine. The
    stage-by-stage form refuses before its first network runs."""
    from instarevive_amd.pipeline import HipTileEngine, process
    from tests.support.small_models import small_models
    swin, vae, dit, y = small_models()
    imgs = [(R.image(1, 128, 192, 70)[0].clamp(0, 1).permute(1, 2, 0) * 255).numpy().astype(np.uint8)]
    with pytest.raises((RuntimeError, ValueError), match="bad tile geometry"):
        process(dit, imgs, 1, "wavelet", False, True, 64, 128, preprocess_model=swin if fused else _NeverCalled(), vae=vae, y=y, y_mask=None, fused=fused)
    if fused:
        eng = HipTileEngine(dit, vae, swin, y, None, "wavelet", False, 64, 128)
        with pytest.raises(ValueError, match="bad tile geometry"):
            eng.count(*imgs[0].shape[:2])
    got, _ = process(dit, imgs, 1, "wavelet", False, True, 64, 64, preprocess_model=swin, vae=vae, y=y, y_mask=None, fused=fused)   # stride == tile stays legal
    assert got[0].shape == imgs[0].shape and len(np.unique(got[0])) > 16
