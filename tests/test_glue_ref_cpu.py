"""The references of tests/support/glue_ref.py (colour fixes, tile blends) pinned to the existing material, the gates of
tests/test_glue_gpu.py derived from the reference's own precision, and every planted bug shown to be caught at the shapes the GPU file runs.

What is pinned: windows() / counts() to oracle.glue.sliding_windows and the five recorded win_* lists; wavelet_fix64 / adain_fix64 to
oracle.glue in float64 (equal to 1e-14 / 1e-12) and to the reference's recorded cf_* outputs; blend32 / to_u8 to the blend loops of
oracle.glue.process driven with recording stand-ins for the four networks (bit-equal, bytes equal).

Yardsticks measured here (max-abs error against the float64 reference; the gate of a case is 4 x its yardstick):
    case        float32 oracle wavelet   adain_apply32
    2x2               8.6e-8                6.4e-7
    8x24              1.7e-7                2.8e-7
    24x8_n3           1.8e-7                3.5e-7
    16x16             1.5e-7                5.8e-7
    64x64_n2          2.6e-7                4.9e-7
    72x200            2.5e-7                1.5e-7
    64x64_n33         2.8e-7                1.7e-7
    mean100             -                   9.4e-6   (9e-8 of the output's magnitude)
    const_style / const_content  -          4.0e-7
The AdaIN figures are led by the flat plane every case carries (std 2e-3 against sqrt(eps) = 3e-3: the rounding of the mean to float32 is
divided by a small std). Without that plane a biased variance does not show at ordinary magnitudes: with both variances far above eps the
factor (n - 1) / n scales the content's and the style's variance alike and cancels (8x24 without it: 0.5 x the gate; 2x2: 219 x).

Planted bugs, the case that catches each best and by how many gates (every one must reach 1.5):
    wavelet  zero padding 2x2 3.7e5; reflect padding 16x16 1.5e5; radius i + 1 16x16 1.5e5;
             four levels 16x16 1.4e5; content / style swapped 2x2 1.9e6; high band from the style 2x2 1.6e6
             both border rules are asserted on both kinds of plane: at 16x16 (an edge <= 16) reflect 1.5e5 and zero 1.6e5, at 72x200 (an edge
             > 32) reflect 4.5e4 and zero 1.6e5
    AdaIN    biased variance 2x2 9.9e3 (8x24: 405, 24x8_n3: 351, 72x200: 10); eps outside the square root 72x200 3.8e5;
             statistics swapped const_style 5.9e7; statistics per item const_style 4.1e5
    blends   (bit-equality; figures in units of the 2-ulp fallback gate) snapped window dropped from the count ragged_y inf (0 / 0);
             count of the other axis even inf; x-major order product / no_overlap 2.2e6; n and tile swapped ragged_y / no_overlap 2.2e6;
             count = number of tiles ragged_y / even 4.7e6; the dropped window changes nothing at even, no_overlap, small_32 (no ragged axis)
    bytes    rounding instead of truncation changes more than 30 % of the bytes of every case
Pixels within 1e-3 of a byte boundary: at most 0.216 % of a frame over all pixel cases (allowed 0.5 %); fp32 and float64 bytes part only there.
Cropped tiles: blend32 gives the frame back exactly at counts 1, 2, 4 and within 1 ulp at 3 and 6; at count 9 (depth 3 in both axes, depth3x3) the
loop's own roundings reach exactly 2 ulp, which is why the crop pass of the GPU file asks 2 ulp at that count and 1 ulp or exactness at the others.
"""
import os

import numpy as np
import pytest
import torch

from oracle import glue as G
from tests.support import glue_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUNDARY_SHARE = 0.005     # pixels within 1e-3 of a byte boundary: at most this share of a frame may differ by 1 from the float64 bytes


def _fx():
    return np.load(os.path.join(GOLD, "glue.npz"))


# ------------------------------------------------------------------------------------------------ the references against the existing material
def test_windows_equal_oracle_and_recorded_lists():
    fx = _fx()
    keys = [k for k in fx.files if k.startswith("win_")]
    assert len(keys) == 5
    for k in keys:
        h, w, t, s = (int(v) for v in k.split("_")[1:])
        assert R.windows(h, w, t, s) == [tuple(int(v) for v in row) for row in fx[k]], k
    for h, w, t, s in R.count_sweep():
        lh, lw, tl, sl = h // 8, w // 8, t // 8, s // 8
        assert R.windows(lh, lw, tl, sl) == G.sliding_windows(lh, lw, tl, sl)
        cnt = torch.zeros(lh, lw, dtype=torch.int64)
        for y, ye, x, xe in R.windows(lh, lw, tl, sl):
            cnt[y:ye, x:xe] += 1
        assert torch.equal(cnt, R.counts(lh, lw, tl, sl)) and int(cnt.min()) >= 1


def test_stride_above_tile_leaves_holes():
    """Why the geometry is refused: latent 16, tile 4, stride 8 gives starts 0, 8, 12 and no window over rows 4 .. 7."""
    assert R.starts(16, 4, 8) == [0, 8, 12]
    c = R.counts(16, 16, 4, 8)
    assert int(c[4:8].max()) == 0 and int(c[0:4, 0:4].min()) == 1


@pytest.mark.parametrize("case", list(R.COLORFIX_CASES))
def test_colour_fix_refs_equal_oracle_in_float64(case):
    c, s = R.colorfix_inputs(*R.COLORFIX_CASES[case])
    c64, s64 = c.double(), s.double()
    assert float((G.wavelet_reconstruction(c64, s64) - R.wavelet_fix64(c, s)).abs().max()) <= 1e-14
    assert float((G.adaptive_instance_normalization(c64, s64) - R.adain_fix64(c, s)).abs().max()) <= 1e-12


def test_colour_fix_refs_reproduce_the_reference_s_recorded_outputs():
    fx = _fx()
    c, s = torch.from_numpy(fx["cf_content"]), torch.from_numpy(fx["cf_style"])
    ew = float((torch.from_numpy(fx["cf_wavelet"]).double() - R.wavelet_fix64(c, s)).abs().max())
    ea = float((torch.from_numpy(fx["cf_adain"]).double() - R.adain_fix64(c, s)).abs().max())
    print(f"reference's recorded fp32 outputs against the float64 references: wavelet {ew:.2e}, adain {ea:.2e}")
    assert ew <= R.wavelet_gate(c, s) and ea <= 2e-6    # the reference's AdaIN is all-fp32 (statistics included): a few ulp of O(1) values


class _StandIns:
    """Identity-like stand-ins for the four networks of oracle.glue.process that record every tile they return."""

    def __init__(self):
        self.x0, self.px = [], []

    def encode(self, x):
        return torch.cat([torch.nn.functional.avg_pool2d(x, 8), x[:, :1, ::8, ::8]], 1)

    def dit(self, lat, t, y, mask):
        k = len(self.x0)
        eps = torch.cat([lat * 0.25 + 0.01 * k, torch.zeros_like(lat)], 1)   # 8 channels: process keeps the first half
        self.x0.append(G.eps_to_mu(self.acp, eps[:, :4], lat, torch.full((1,), 400).long()))
        return eps

    def decode(self, z):
        k = len(self.px)
        out = torch.nn.functional.interpolate(z[:, :3], scale_factor=8, mode="nearest") - 0.5 + 0.02 * k
        self.px.append(out / 2 + 0.5)
        return out


@pytest.mark.parametrize("h,w,tile,stride", [(192, 256, 64, 48), (128, 192, 64, 40), (192, 192, 64, 40)])
def test_blend_refs_equal_the_blend_loops_of_oracle_process(h, w, tile, stride):
    n = 2
    imgs = [(R.image(1, h, w, 50 + i)[0].clamp(0, 1).permute(1, 2, 0) * 255).numpy().astype(np.uint8) for i in range(n)]
    st = _StandIns()
    st.acp = G.alphas_cumprod()
    preds, _, inter = G.process(imgs, lambda x: x, st.encode, st.dit, st.decode, st.acp, None, None, scaling_factor=1.0, color_fix_type="none",
                                tiled=True, tile_size=tile, tile_stride=stride, return_intermediates=True)
    lh, lw, tl, sl = h // 8, w // 8, tile // 8, stride // 8
    K = len(R.windows(lh, lw, tl, sl))
    assert len(st.x0) == K and len(st.px) == K
    x0, px = torch.stack(st.x0, 0), torch.stack(st.px, 0)
    assert torch.equal(inter["x0"], R.blend32(x0, n, 4, lh, lw, tl, sl))
    img32 = R.blend32(px, n, 3, h, w, tile, stride)
    assert torch.equal(inter["img"], img32)
    assert np.array_equal(preds, R.to_u8(img32).numpy())
    assert float((R.blend64(x0, n, 4, lh, lw, tl, sl) - inter["x0"].double()).abs().max()) <= 1e-6
    assert len(np.unique(preds)) > 100    # the stand-ins made a picture, not a clamped plane


def _crop_pass(case, ch):
    """Tiles cropped from one frame, blended by the fp32 loop: (error in ulp of the frame's value, count), per element."""
    n, h, w, tile, stride = R.BLEND_CASES[case]
    if ch == 4:
        h, w, tile, stride = h // 8, w // 8, tile // 8, stride // 8
    frame = R.image(n, h, w, 9, ch)
    got = R.blend32(R.crop_tiles(frame, tile, stride), n, ch, h, w, tile, stride)
    return (got.double() - frame.double()).abs() / R.ulp32(frame), R.counts(h, w, tile, stride).expand_as(frame)


def test_blend32_gives_cropped_tiles_back_exactly_at_counts_1_2_4_and_within_1_ulp_up_to_count_6():
    """The bounds of the GPU file's crop pass (R.CROP_ULP) hold for the fp32 loop itself, and the 2 ulp at count 9 are reached: no blend in loop
    order can promise 1 ulp there."""
    seen = set()
    for case in R.CROP_CASES:
        for ch in (4, 3):
            err, cnt = _crop_pass(case, ch)
            seen |= set(cnt.flatten().tolist())
            for k in sorted(set(cnt.flatten().tolist())):
                assert float(err[cnt == k].max()) <= R.CROP_ULP[k], (case, ch, k)
    assert seen == set(R.CROP_ULP) == {1, 2, 3, 4, 6, 9}
    assert all(R.CROP_ULP[k] == 0.0 for k in (1, 2, 4)) and all(R.CROP_ULP[k] == 1.0 for k in (3, 6))
    err, cnt = _crop_pass("depth3x3", 3)
    assert sorted(set(cnt.flatten().tolist())) == [1, 2, 3, 4, 6, 9]
    assert float(err[cnt == 9].max()) == 2.0 == R.CROP_ULP[9] and float(err[cnt != 9].max()) <= 1.0


# ------------------------------------------------------------------------------------------------ gates and planted bugs
def _colorfix_cases(kind):
    cases = {k: R.colorfix_inputs(*v) for k, v in R.COLORFIX_CASES.items()}
    if kind == "adain":
        cases.update({k: R.adain_special_inputs(k) for k in R.ADAIN_SPECIAL})
    return cases


def _separations(kind):
    ref, gate, bugs = {"wavelet": (R.wavelet_fix64, R.wavelet_gate, R.WAVELET_BUGS), "adain": (R.adain_fix64, R.adain_gate, R.ADAIN_BUGS)}[kind]
    best = {b: (0.0, None) for b in bugs}
    gates = {}
    for name, (c, s) in _colorfix_cases(kind).items():
        want = ref(c, s)
        gates[name] = gate(c, s)
        for b in bugs:
            sep = float((ref(c, s, bug=b) - want).abs().max()) / gates[name]
            print(f"{kind} {name}: gate {gates[name]:.2e}, bug {b} at {sep:.3g} x the gate")
            if sep > best[b][0]:
                best[b] = (sep, name)
    return gates, best


def test_wavelet_gates_and_planted_bugs():
    gates, best = _separations("wavelet")
    # yardstick of the float32 oracle: a few ulp of O(1) values at every size
    assert all(4 * 5e-8 <= g <= 4 * 5e-7 for g in gates.values()), gates
    for b, (sep, name) in best.items():
        print(f"wavelet bug {b}: caught best by {name} at {sep:.3g} x its gate")
        assert sep >= R.SEPARATION, (b, sep)
    # each border rule is caught both on a plane no wider than the largest radius (an edge <= 16) and on one wider than twice it (an edge > 32)
    for name in ("16x16", "72x200"):
        c, s = R.colorfix_inputs(*R.COLORFIX_CASES[name])
        want = R.wavelet_fix64(c, s)
        for b in ("reflect_pad", "zero_pad"):
            sep = float((R.wavelet_fix64(c, s, bug=b) - want).abs().max()) / gates[name]
            print(f"wavelet {b} at {name}: {sep:.3g} x the gate")
            assert sep >= R.SEPARATION, (name, b, sep)


def test_adain_gates_and_planted_bugs():
    gates, best = _separations("adain")
    # a few ulp of O(1) values; the flat plane of every case (std 2e-3 against sqrt(eps) = 3e-3) amplifies the rounding of c - mean
    assert all(g <= 4 * 1e-6 for k, g in gates.items() if k != "mean100"), gates
    assert gates["mean100"] <= 4 * 4 * 7.63e-6            # a few ulp of 100
    for b, (sep, name) in best.items():
        print(f"adain bug {b}: caught best by {name} at {sep:.3g} x its gate")
        assert sep >= R.SEPARATION, (b, sep)
    # the biased variance is the reason for the two small planes: it must be caught there, at ordinary magnitudes
    for name in ("2x2", "8x24", "24x8_n3"):
        c, s = R.colorfix_inputs(*R.COLORFIX_CASES[name])
        sep = float((R.adain_fix64(c, s, bug="biased_var") - R.adain_fix64(c, s)).abs().max()) / gates[name]
        print(f"adain biased variance at {name}: {sep:.3g} x the gate")
        assert sep >= R.SEPARATION
    # ... and is out of reach of any fp32 gate at the tile the product runs
    c, s = R.colorfix_inputs(1, 512, 512)
    assert float((R.adain_fix64(c, s, bug="biased_var") - R.adain_fix64(c, s)).abs().max()) < 1e-5


@pytest.mark.parametrize("ch", [4, 3])
def test_planted_blend_bugs_change_the_bits(ch):
    best = {b: (0.0, None) for b in R.BLEND_BUGS}
    for case in R.BLEND_CASES:
        if case == "product" and ch == 3:
            continue
        tiles, geo = R.blend_tiles(case, ch)
        want = R.blend32(tiles, *geo)
        two_ulp = 2 * float(R.ulp32(want.abs().max()))      # the fallback gate, should the GPU division not be bit-equal
        for b in R.BLEND_BUGS:
            got = R.blend32(tiles, *geo, bug=b)
            d = (got.double() - want.double()).abs()
            sep = float(torch.nan_to_num(d, nan=float("inf"), posinf=float("inf")).max()) / two_ulp
            if sep > best[b][0]:
                best[b] = (sep, case)
    for b, (sep, case) in best.items():
        print(f"blend ({ch} channels) bug {b}: caught best by {case} at {sep:.3g} x 2 ulp")
        assert sep >= R.SEPARATION, (b, sep)


def test_snapped_window_bug_needs_a_ragged_axis():
    for case, caught in (("even", False), ("no_overlap", False), ("small_32_n1", False), ("ragged_y", True), ("ragged_x", True), ("small_40_n1", True)):
        tiles, geo = R.blend_tiles(case, 4)
        same = torch.equal(R.blend32(tiles, *geo, bug="snapped_window_dropped"), R.blend32(tiles, *geo))
        assert same != caught, case
    for case, axis in (("ragged_y", 0), ("ragged_x", 1)):    # ragged in exactly one axis: the wrong count depends on that coordinate alone
        _, h, w, t, s = R.BLEND_CASES[case]
        bad = R.counts(h // 8, w // 8, t // 8, s // 8, bug="snapped_window_dropped") != R.counts(h // 8, w // 8, t // 8, s // 8)
        line = bad.select(1 - axis, 0)
        assert bool(line.any()) and not bool(line.all()) and torch.equal(bad, line.unsqueeze(1 - axis).expand_as(bad))


def test_pixel_inputs_keep_the_byte_boundary_share_and_rounding_is_caught():
    worst = 0.0
    for case in R.BLEND_CASES:
        tiles, geo = R.blend_tiles(case, 3)
        b64, b32 = R.blend64(tiles, *geo), R.blend32(tiles, *geo)
        near = R.u8_boundary(b64)
        share = float(near.double().mean())
        worst = max(worst, share)
        u64, u32 = R.to_u8(b64), R.to_u8(b32)
        diff = u64 != u32
        assert share <= BOUNDARY_SHARE, (case, share)
        assert not bool((diff & ~near).any()), case                  # fp32 and float64 bytes part only at a boundary ...
        assert int((u64.int() - u32.int()).abs().max()) <= 1         # ... and then by one
        rounded = float((R.to_u8(b32, bug="round_to_u8") != u32).double().mean())
        assert rounded >= R.SEPARATION * BOUNDARY_SHARE and rounded > 0.3, (case, rounded)
        clamped = float(((b64 <= 0) | (b64 >= 1)).double().mean())
        assert clamped > 0.01, case                                  # values on both sides of [0, 1] survive the blend
    print(f"largest share of pixels within 1e-3 of a byte boundary: {100 * worst:.3f} % (allowed {100 * BOUNDARY_SHARE} %)")


# ------------------------------------------------------------------------------------------------ the host side of the library (no GPU needed)
def test_ir_tiled_count_equals_the_window_list_and_refuses_bad_geometry():
    from instarevive_amd import _lib as L
    lib = L.load_library()
    for h, w, t, s in R.count_sweep():
        assert lib.ir_tiled_count(h, w, t, s) == len(R.windows(h // 8, w // 8, t // 8, s // 8)), (h, w, t, s)
    for why, geo in R.BAD_GEOMETRIES.items():
        assert lib.ir_tiled_count(*geo) == -31, why
    assert lib.ir_tiled_count(2176, 3840, 512, 1024) == -31          # --tile_size 512 --tile_stride 1024 used to write black stripes
