"""References for the glue between the networks and the picture: the colour fixes (ir_color_fix) and the tile blends (ir_tiled_count,
ir_tiled_blend_latent, ir_tiled_blend_pixels). Plain torch in float64, device-agnostic (they run where their inputs live), written from
the definitions and not from the kernels: index clamps and nine shifted adds for the a-trous blur, sum over count for the blends.

Next to them the fp32 emulations that serve as yardsticks (adain_apply32) and as the bit-exact form of the blends (blend32), and the
planted bugs: every reference takes `bug=<name>` and then computes what a subtly wrong kernel would. tests/test_glue_ref_cpu.py pins the
references to oracle.glue and to the recorded outputs of the reference, derives the gates and shows that every planted bug is caught at
the shapes tests/test_glue_gpu.py runs."""
import numpy as np
import torch

WAVELET_BUGS = ("zero_pad", "reflect_pad", "radius_i_plus_1", "four_levels", "swapped", "high_from_style")
ADAIN_BUGS = ("biased_var", "eps_outside_sqrt", "stats_swapped", "stats_per_item")
BLEND_BUGS = ("snapped_window_dropped", "count_of_other_axis", "x_major_order", "n_tile_swapped", "count_is_tiles")
U8_BUGS = ("round_to_u8",)

# ir_color_fix cases, n x h x w (the 32 x 512 x 512 launch of decode_tiles_run is "product" in the GPU file: too large for the CPU file)
COLORFIX_CASES = {"2x2": (1, 2, 2), "8x24": (1, 8, 24), "24x8_n3": (3, 24, 8), "16x16": (1, 16, 16), "64x64_n2": (2, 64, 64),
                  "72x200": (1, 72, 200), "64x64_n33": (33, 64, 64)}
COLORFIX_PRODUCT = (32, 512, 512)
PRODUCT_BASE = 2         # the product case is PRODUCT_BASE drawn items, repeated with a gain and an offset of their own (product_inputs)
PRODUCT_GATE_ITEMS = (0, 1, 30, 31)   # the items of the product case on which its wavelet yardstick is taken (product_wavelet_gate)
ADAIN_SPECIAL = ("mean100", "const_style", "const_content")   # 1 x 24 x 40 each, plane 1 is the special one

# tile geometries: n, frame h x w, tile, stride (pixels; frames multiples of 64, tile / 8 even)
BLEND_CASES = {
    "even": (1, 192, 256, 64, 32),            # ragged in neither axis
    "ragged_y": (2, 192, 256, 64, 48),        # (24 - 8) % 6 = 4, (32 - 8) % 6 = 0
    "ragged_x": (2, 256, 192, 64, 48),
    "tile_is_height": (1, 128, 320, 128, 48),
    "no_overlap": (2, 192, 256, 64, 64),
    "depth3": (1, 192, 64, 64, 40),           # 24 / 8 / 5 in latent units: starts 0, 5, 10, 15, 16, up to 3 windows over a pixel
    "depth3x3": (1, 192, 192, 64, 40),        # the same in both axes: counts 1, 2, 3, 4, 6, 9
    # 64 / 40 on 128 x 192 is ragged in both axes ((16 - 8) % 5 = 3, (24 - 8) % 5 = 1), 64 / 32 in neither
    "small_40_n1": (1, 128, 192, 64, 40), "small_40_n2": (2, 128, 192, 64, 40), "small_40_n3": (3, 128, 192, 64, 40),
    "small_32_n1": (1, 128, 192, 64, 32), "small_32_n2": (2, 128, 192, 64, 32), "small_32_n3": (3, 128, 192, 64, 32),
    "product": (2, 1088, 1536, 512, 448),
}

# second pass (tiles cropped from one frame blend back to it), every geometry of the list: exactly where the count is 1, 2 or 4, within 1 ulp
# of the frame's value at counts 3 and 6. At count 9 (depth3x3 alone) the fp32 loop itself (blend32: eight roundings of sums of up to 9 v, then
# the division) is 2 ulp off, see tests/test_glue_ref_cpu.py, so no blend in loop order can promise 1 ulp there: 2 ulp at that count.
CROP_CASES = tuple(BLEND_CASES)
CROP_ULP = {1: 0.0, 2: 0.0, 4: 0.0, 3: 1.0, 6: 1.0, 9: 2.0}


# ------------------------------------------------------------------------------------------------ inputs
def image(n, h, w, seed, ch=3):
    """A smooth colour field plus noise of std 0.15 (uniform, numpy PCG64 as tests/golden/_det.py draws): float32 [n, ch, h, w] with values
    on both sides of [0, 1]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy = np.linspace(0.0, 1.0, h, dtype=np.float64)[:, None]
    xx = np.linspace(0.0, 1.0, w, dtype=np.float64)[None, :]
    planes = [0.5 + 0.4 * np.sin(7 * xx + 3 * yy), 0.5 + 0.4 * np.cos(5 * yy - 2 * xx), 0.3 + 0.5 * xx * yy, 0.6 - 0.4 * xx + 0.2 * yy]
    base = np.stack([planes[c % 4] for c in range(ch)], 0)
    a = 0.15 * 3.0 ** 0.5
    noise = rng.random(size=(n, ch, h, w), dtype=np.float64) * (2 * a) - a
    return torch.from_numpy((base[None] + noise).astype(np.float32))


def colorfix_inputs(n, h, w, seed=1):
    """Content and style of a colour-fix case. The blue plane of the last content item is flat (contrast 1 %, std about 2e-3, a patch of sky):
    only where a plane's variance is of the size of AdaIN's eps = 1e-5 does the variance estimator show in the result - with both variances
    far above eps a biased estimate scales numerator and denominator alike and cancels."""
    c, s = image(n, h, w, seed), image(n, h, w, seed + 1000) * 0.8 + 0.1
    c[-1, 2] = 0.5 + (c[-1, 2] - 0.5) * 0.01
    return c, s


def product_inputs(device):
    """The colour-fix launch of decode_tiles_run at tile 512: 32 items, (content, style) on `device`. PRODUCT_BASE items are drawn, the others
    repeat them with a gain of at most 1.08 and an offset of at most 0.05 of their own, so that no two items are equal."""
    n, h, w = COLORFIX_PRODUCT
    bc, bs = colorfix_inputs(PRODUCT_BASE, h, w, seed=3)
    rep = torch.arange(n, device=device) // PRODUCT_BASE
    gain, off = (1 + 0.005 * rep).float()[:, None, None, None], (0.003 * rep).float()[:, None, None, None]
    c = bc.to(device).repeat(n // PRODUCT_BASE, 1, 1, 1) * gain + off
    s = bs.to(device).repeat(n // PRODUCT_BASE, 1, 1, 1) * gain - off
    return c.contiguous(), s.contiguous()


def adain_special_inputs(kind):
    c, s = colorfix_inputs(1, 24, 40, seed=7)
    if kind == "mean100":          # mean 100, std 1e-3 on both sides: a float32 variance by sum of squares would be noise
        c[:, 1] = (c[:, 1] - 0.5) * (1e-3 / 0.28) + 100.0
        s[:, 1] = (s[:, 1] - 0.5) * (2e-3 / 0.24) + 100.0
    elif kind == "const_style":    # std exactly sqrt(1e-5)
        s[:, 1] = 0.25
    elif kind == "const_content":
        c[:, 1] = 0.75
    else:
        raise KeyError(kind)
    return c, s


# ------------------------------------------------------------------------------------------------ windows
def starts(size, tile, stride):
    v = list(range(0, size - tile + 1, stride))
    if (size - tile) % stride != 0:
        v.append(size - tile)
    return v


def windows(h, w, tile, stride):
    """The reference's _sliding_windows list (hi, he, wi, we) in its loop order: rows outside, columns inside."""
    return [(y, y + tile, x, x + tile) for y in starts(h, tile, stride) for x in starts(w, tile, stride)]


def _axis_count(length, size, tile, stride, drop_snapped=False):
    """How many window starts of an axis of `size` cover each of the positions 0 .. length - 1."""
    st = starts(size, tile, stride)
    if drop_snapped and (size - tile) % stride != 0:
        st = st[:-1]
    c = torch.zeros(length, dtype=torch.int64)
    for s in st:
        c[max(0, min(s, length)):max(0, min(s + tile, length))] += 1
    return c


def counts(h, w, tile, stride, bug=None):
    """Overlap count per pixel, int64 [h, w]."""
    if bug == "count_of_other_axis":
        return _axis_count(h, w, tile, stride)[:, None] * _axis_count(w, h, tile, stride)[None, :]
    if bug == "count_is_tiles":
        return torch.full((h, w), len(windows(h, w, tile, stride)), dtype=torch.int64)
    drop = bug == "snapped_window_dropped"
    return _axis_count(h, h, tile, stride, drop)[:, None] * _axis_count(w, w, tile, stride, drop)[None, :]


# ------------------------------------------------------------------------------------------------ wavelet colour fix
def _shift_index(size, off, pad, device):
    """Source index and validity of position + off along an axis of `size` under the border rule."""
    i = torch.arange(size, device=device) + off
    valid = (i >= 0) & (i < size)
    if pad == "reflect":
        if size == 1:
            i = torch.zeros_like(i)
        else:
            p = 2 * (size - 1)
            i = i % p
            i = torch.where(i >= size, p - i, i)
    else:
        i = i.clamp(0, size - 1)
    return i, valid


def blur64(img, radius, pad="replicate"):
    """[1,2,1] x [1,2,1] / 16 at dilation `radius`: nine weighted shifted adds; works for radius >= plane size."""
    H, W = img.shape[-2:]
    out = torch.zeros_like(img)
    for dy in (-1, 0, 1):
        iy, vy = _shift_index(H, dy * radius, pad, img.device)
        rows = img.index_select(-2, iy)
        if pad == "zero":
            rows = rows * vy.to(img.dtype)[:, None]
        for dx in (-1, 0, 1):
            ix, vx = _shift_index(W, dx * radius, pad, img.device)
            tap = rows.index_select(-1, ix)
            if pad == "zero":
                tap = tap * vx.to(img.dtype)[None, :]
            out += tap * ((0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25))
    return out


def wavelet_decomposition64(img, levels=5, pad="replicate", radius=lambda i: 2 ** i):
    high = torch.zeros_like(img)
    low = img
    for i in range(levels):
        low = blur64(img, radius(i), pad)
        high += img - low
        img = low
    return high, low


def wavelet_fix64(content, style, bug=None):
    """high(content) + low(style), five a-trous levels at radius 2**i, replicate border; float64 on the inputs' device."""
    c, s = content.to(torch.float64), style.to(torch.float64)
    kw = {}
    if bug == "zero_pad":
        kw["pad"] = "zero"
    elif bug == "reflect_pad":
        kw["pad"] = "reflect"
    elif bug == "radius_i_plus_1":
        kw["radius"] = lambda i: i + 1
    elif bug == "four_levels":
        kw["levels"] = 4
    elif bug == "swapped":
        c, s = s, c
    elif bug == "high_from_style":
        c = s
    elif bug is not None:
        raise KeyError(bug)
    return wavelet_decomposition64(c, **kw)[0] + wavelet_decomposition64(s, **kw)[1]


# ------------------------------------------------------------------------------------------------ AdaIN colour fix
def plane_stats64(x, bug=None):
    """Per-plane mean and sqrt(unbiased variance + 1e-5), float64 [n, ch, 1, 1] each."""
    x = x.to(torch.float64)
    n, ch = x.shape[:2]
    f = x.reshape(n, 1, -1).expand(n, ch, -1) if bug == "stats_per_item" else x.reshape(n, ch, -1)
    m = f.mean(2)
    v = f.var(2, unbiased=bug != "biased_var")
    sd = v.sqrt() + 1e-5 if bug == "eps_outside_sqrt" else (v + 1e-5).sqrt()
    return m.reshape(n, ch, 1, 1), sd.reshape(n, ch, 1, 1)


def adain_fix64(content, style, bug=None):
    if bug is not None and bug not in ADAIN_BUGS:
        raise KeyError(bug)
    c, s = content.to(torch.float64), style.to(torch.float64)
    cm, cs = plane_stats64(c, bug)
    sm, ss = plane_stats64(s, bug)
    if bug == "stats_swapped":
        cm, cs, sm, ss = sm, ss, cm, cs
    return (c - cm) / cs * ss + sm


def adain_apply32(content, style):
    """The yardstick of an fp32 implementation: float64 statistics rounded to float32, applied in float32 (one rounding per operation)."""
    cm, cs = (t.to(torch.float32) for t in plane_stats64(content))
    sm, ss = (t.to(torch.float32) for t in plane_stats64(style))
    return (content.to(torch.float32) - cm) / cs * ss + sm


# ------------------------------------------------------------------------------------------------ tile blends
def _placed(tiles, n, ch, H, W, tile, stride, bug):
    """(tile tensor [n, ch, t, t], y, x) in accumulation order; `tiles` is the ABI's [tile][n][ch][t][t]."""
    wins = windows(H, W, tile, stride)
    K = len(wins)
    assert tuple(tiles.shape) == (K, n, ch, tile, tile), (tuple(tiles.shape), (K, n, ch, tile, tile))
    if bug == "n_tile_swapped":
        tiles = tiles.reshape(n, K, ch, tile, tile).transpose(0, 1)
    offs = [(y, x) for y, _, x, _ in wins]
    if bug == "x_major_order":
        offs = [(y, x) for x in starts(W, tile, stride) for y in starts(H, tile, stride)]
    return [(tiles[i], offs[i][0], offs[i][1]) for i in range(K)]


def _blend(tiles, n, ch, H, W, tile, stride, bug, dtype):
    if bug is not None and bug not in BLEND_BUGS:
        raise KeyError(bug)
    buf = torch.zeros((n, ch, H, W), dtype=dtype, device=tiles.device)
    for t, y, x in _placed(tiles, n, ch, H, W, tile, stride, bug):   # strictly in loop order, one add per tile
        buf[:, :, y:y + tile, x:x + tile] += t.to(dtype)
    return buf / counts(H, W, tile, stride, bug).to(device=tiles.device, dtype=dtype)


def blend64(tiles, n, ch, H, W, tile, stride, bug=None):
    """Sum over count in float64; sizes in the units of the tiles (latent pixels for the latent blend, pixels for the pixel blend)."""
    return _blend(tiles, n, ch, H, W, tile, stride, bug, torch.float64)


def blend32(tiles, n, ch, H, W, tile, stride, bug=None):
    """What an fp32 blend must give to the bit: float32 adds in loop order from a zero buffer, then one IEEE division by the float count."""
    return _blend(tiles.to(torch.float32), n, ch, H, W, tile, stride, bug, torch.float32)


def to_u8(img, bug=None):
    """[n, 3, H, W] -> uint8 [n, H, W, 3]: clamp(0, 1) * 255 truncated, in the precision of `img`."""
    v = img.clamp(0, 1) * 255
    v = torch.floor(v + 0.5).clamp(0, 255) if bug == "round_to_u8" else torch.floor(v)
    return v.permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def u8_boundary(img64, tol=1e-3):
    """Pixels whose float64 value * 255 lies within tol of an integer, clamped values aside: there truncating an fp32 blend may land on the
    neighbouring byte. bool [n, H, W, 3]."""
    v = img64.to(torch.float64).clamp(0, 1) * 255
    near = (v - torch.round(v)).abs() < tol
    inside = (img64 > 0) & (img64 < 1)
    return (near & inside).permute(0, 2, 3, 1).contiguous()


def blend_tiles(case, ch, seed0=100):
    """Every tile with content of its own (image() seeded by the tile index), [tile][n][ch][t][t] float32, sizes in units of the tiles."""
    n, h, w, tile, stride = BLEND_CASES[case]
    if ch == 4:
        h, w, tile, stride = h // 8, w // 8, tile // 8, stride // 8
    K = len(windows(h, w, tile, stride))
    return torch.stack([image(n, tile, tile, seed0 + i, ch) for i in range(K)], 0), (n, ch, h, w, tile, stride)


def crop_tiles(frame, tile, stride):
    """The tiles of one frame [n, ch, H, W] in loop order."""
    H, W = frame.shape[-2:]
    return torch.stack([frame[:, :, y:ye, x:xe] for y, ye, x, xe in windows(H, W, tile, stride)], 0).contiguous()


def ulp32(x):
    """Spacing of float32 at |x| (float64 tensor)."""
    x = x.to(torch.float64).abs().clamp_min(2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(x)) - 23)


# ------------------------------------------------------------------------------------------------ gates (measured against the reference, never the HIP result)
GATE_FACTOR = 4.0        # over the fp32 yardstick's own max-abs error: room for another order of the nine adds over five levels
SEPARATION = 1.5         # every planted bug must land at least this far outside the gate of one case


def wavelet_gate(content, style):
    """GATE_FACTOR x the max-abs error of the float32 oracle.glue.wavelet_reconstruction against wavelet_fix64 on these inputs (CPU)."""
    from oracle import glue as G
    c, s = content.cpu().float(), style.cpu().float()
    return GATE_FACTOR * float((G.wavelet_reconstruction(c, s).double() - wavelet_fix64(c, s)).abs().max())


def product_wavelet_gate(content, style):
    """The wavelet gate of the 32 x 512 x 512 case: wavelet_gate on four of the 32 items the kernel receives, the first and the last pair (smallest
    and largest gain). The float32 oracle is a dilated CPU convolution that takes most of a second per 512 x 512 item, so all 32 would cost this one
    case half a minute. The maximum over a subset cannot exceed the maximum over all items: the gate is never wider than the one over all 32."""
    i = list(PRODUCT_GATE_ITEMS)
    return wavelet_gate(content[i], style[i])


def adain_gate(content, style):
    """GATE_FACTOR x the max-abs error of adain_apply32 against adain_fix64 on these inputs, computed where they live. The kernel keeps its
    statistics in double, so the float32 oracle (off by up to 1e-3 on a plane of mean 100, std 1e-3) is not the yardstick."""
    c, s = content.float(), style.float()
    return GATE_FACTOR * float((adain_apply32(c, s).double() - adain_fix64(c, s)).abs().max())


def count_sweep():
    """A few hundred valid (h, w, tile, stride) in pixels for ir_tiled_count: every stride from 8 to the tile, tiles up to the frame."""
    out = []
    for h, w in ((64, 64), (64, 192), (128, 192), (192, 128), (192, 320), (320, 256)):
        for tile in (16, 32, 48, 64, 96, 128, 192):
            if tile > min(h, w):
                continue
            for stride in range(8, tile + 1, 8):
                out.append((h, w, tile, stride))
    out += [(2176, 3840, 512, 448), (1088, 1536, 512, 448), (2048, 2048, 512, 448), (1024, 1536, 512, 448), (512, 512, 512, 512)]
    return out


# refused geometries (h, w, tile, stride) -> why
BAD_GEOMETRIES = {
    "odd_tile_over_8": (192, 256, 72, 32),
    "tile_above_frame": (128, 256, 192, 64),
    "stride_below_8": (192, 256, 64, 7),
    "stride_above_tile": (128, 128, 32, 64),   # latent 16, tile 4, stride 8: starts 0, 8, 12 leave rows 4 .. 7 uncovered
}
