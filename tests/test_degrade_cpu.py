"""The host side of --degrade (instarevive_amd/degrade.py) and its definition (tools/degrade_folder.py), without a GPU.

The JPEG model is held to Pillow (libjpeg) byte for byte - an equality, no tolerance - on twenty sizes x nine qualities x two kinds of
content; the blur-kernel builder to the reference's own bivariate_Gaussian (tests/golden/degrade.npz, made by make_degrade_golden.py) at 1e-15
relative, both being float64 numpy; the noise step to the reference's add_gaussian_noise bit for bit."""
import argparse
import json
import os

import numpy as np
import pytest

from instarevive_amd import degrade as D
from tests.support import degrade_model as DM
from tools import degrade_folder as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (8, 16), (16, 8), (8, 24), (24, 8), (12, 12), (15, 15), (16, 16), (16, 17), (17, 23), (33, 16), (9, 40), (40, 9), (1, 1), (3, 50),
         (32, 48), (37, 53), (64, 41), (128, 128), (200, 311)]
QUALITIES = (10, 30, 35, 60, 75, 77, 90, 95, 100)


def _content(kind, h, w):
    rng = np.random.default_rng([h, w, len(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    walk = np.cumsum(np.cumsum(rng.normal(0, 1.5, (h, w, 3)), 0), 1) * 0.3
    return np.clip(128 + walk, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- the JPEG model against Pillow
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_jpeg_model_equals_pillow_byte_for_byte(size):
    for kind in ("noise", "smooth"):
        img = _content(kind, *size)
        for q in QUALITIES:
            ref, got = DM.pillow_roundtrip(img, q), M.jpeg_roundtrip(img, q)
            assert np.array_equal(ref, got), (size, kind, q, int(np.abs(ref.astype(int) - got).max()), np.argwhere(ref != got)[:4])


def test_library_quant_tables_equal_the_models():
    import ctypes as C
    from instarevive_amd import _lib as L
    lib = L.load_library()
    for q in (1, 10, 49, 50, 75, 100):
        lu, ch = np.zeros(64, dtype=np.uint16), np.zeros(64, dtype=np.uint16)
        assert lib.ir_degrade_qtables(q, C.c_void_p(lu.ctypes.data), C.c_void_p(ch.ctypes.data)) == 0
        ml, mc = M.quant_tables(q)
        assert np.array_equal(lu.reshape(8, 8), ml) and np.array_equal(ch.reshape(8, 8), mc)
    assert lib.ir_degrade_qtables(0, C.c_void_p(lu.ctypes.data), C.c_void_p(ch.ctypes.data)) == -1
    assert lib.ir_degrade_qtables(101, C.c_void_p(lu.ctypes.data), C.c_void_p(ch.ctypes.data)) == -1


def test_unit_scale_has_one_value_per_byte():
    """Step 1 rounds v / 255.0 from double, step 5 divides float32 by float32: the kernel uses one function for both, so they must agree."""
    v = np.arange(256)
    assert np.array_equal((v / 255.0).astype(np.float32), v.astype(np.float32) / np.float32(255.0))
    x = (v / 255.0).astype(np.float32)
    assert np.array_equal(np.rint(x * np.float32(255.0)), v) and np.array_equal((x * np.float32(255.0)).astype(np.uint8), v)


# ---------------------------------------------------------------- kernel builder and noise against the reference's outputs
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade.npz"))


def test_blur_kernel_equals_the_reference(golden):
    cases = golden["cases"]
    assert len(cases) >= 6
    assert any(c[0] == 41 and c[1] == 0.1 for c in cases) and any(c[0] == 41 and c[1] == 10 for c in cases)
    for i, (K, sx, sy, th, iso) in enumerate(cases):
        ref = golden[f"kernel_{i}"]
        got = D.bivariate_gaussian(int(K), sx, sy, th, bool(iso))
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.all(np.abs(got - ref) <= 1e-15 * np.abs(ref)), (i, float(np.abs(got - ref).max()))
        assert abs(got.sum() - 1.0) < 1e-12


def test_noise_step_equals_the_reference(golden):
    got = M.add_noise(golden["noise_img"], golden["noise_field"], float(golden["noise_sigma"]))
    assert got.dtype == np.float32 and np.array_equal(got, golden["noise_out"])


# ---------------------------------------------------------------- recipe and sampler
def test_same_file_and_seed_give_the_same_record_in_any_order():
    rec = D.load_recipe("lq")
    names = [f"sub/img_{i}.png" for i in range(6)]
    first = {n: D.draw(rec, n, 96, 128, 231) for n in names}
    for n in reversed(names):
        p, q = D.draw(rec, n, 96, 128, 231), first[n]
        assert (p.lh, p.lw, p.sigma, p.q, p.norm, p.scale, p.kind) == (q.lh, q.lw, q.sigma, q.q, q.norm, q.scale, q.kind)
        assert np.array_equal(p.kernel, q.kernel) and np.array_equal(p.noise, q.noise)
    assert len({(p.scale, p.sigma) for p in first.values()}) == len(names)   # files differ
    other = D.draw(rec, names[0], 96, 128, 232)
    assert (other.scale, other.sigma) != (first[names[0]].scale, first[names[0]].sigma)   # seeds differ
    assert D.draw(rec, "sub\\img_0.png", 96, 128, 231).scale == first["sub/img_0.png"].scale   # one name on every platform


def test_draws_stay_inside_the_recipe():
    rec = D.load_recipe("lq")
    kinds = set()
    for i in range(200):
        p = D.draw(rec, f"{i}.png", 128, 160, 7)
        kinds.add(p.kind)
        assert 2 <= p.scale <= 4 and (p.lh, p.lw) == (int(128 // p.scale), int(160 // p.scale))
        assert 0 <= p.sigma <= 20 and 60 <= p.q <= 100 and p.norm == M.NORM_NONE
        assert p.kernel.shape == (41, 41) and p.kernel.dtype == np.float64 and abs(p.kernel.sum() - 1) < 1e-12 and p.kernel.min() >= 0
        assert p.noise.shape == (p.lh, p.lw, 3) and p.noise.dtype == np.float32
        assert p.noise.size * 4 <= 128 * 160 * 3   # at most a quarter of the image's pixels
        D.check_params(p, 128, 160)
    assert kinds == {"iso", "aniso"}


def test_recipe_file_and_refusals(tmp_path):
    f = tmp_path / "r.json"
    f.write_text(json.dumps({"blur_kernel_size": 21, "kernel_list": ["iso"], "kernel_prob": [1], "blur_sigma": [1, 2], "downsample_range": [1, 1],
                             "noise_range": None, "jpeg_range": None, "norm": "max"}))
    p = D.draw(D.load_recipe(str(f)), "a.png", 40, 40, 1)
    assert p.kernel.shape == (21, 21) and p.kind == "iso" and p.noise is None and p.q == 0 and p.norm == M.NORM_MAX and (p.lh, p.lw) == (40, 40)
    for kind in ("generalized_iso", "plateau_aniso", "skew"):
        with pytest.raises(D.DegradeError, match=f"kernel type `{kind}` is not supported"):
            D.load_recipe({"kernel_list": ["iso", kind], "kernel_prob": [0.5, 0.5]})
    with pytest.raises(D.DegradeError, match="blur_kernel_size"):
        D.load_recipe({"blur_kernel_size": 43})
    with pytest.raises(D.DegradeError, match="unknown keys"):
        D.load_recipe({"blur_kernel": 41})
    with pytest.raises(D.DegradeError, match="too small"):
        D.draw(D.load_recipe("lq"), "a.png", 20, 64, 1)
    with pytest.raises(D.DegradeError, match="below 8 pixels"):
        D.draw(D.load_recipe({"downsample_range": [4, 4]}), "a.png", 30, 64, 1)


@pytest.mark.parametrize("flag", ["show_lq", "use_center_crop", "shard_tiles"])
def test_conflicting_flags_are_refused_by_name(flag):
    args = argparse.Namespace(show_lq=False, use_center_crop=False, shard_tiles=False)
    D.check_flags(args)
    setattr(args, flag, True)
    with pytest.raises(D.DegradeError, match=f"--{flag}"):
        D.check_flags(args)


# ---------------------------------------------------------------- the whole model
def test_identity_settings_reproduce_the_input():
    img = DM.image(37, 53)
    for K in (1, 41):
        for norm in (M.NORM_NONE,):
            out = M.degrade_model(img, D.delta_kernel(K), 37, 53, 0.0, 0, None, norm)
            assert np.array_equal(out, img), K
    zero_sigma = M.degrade_model(img, D.delta_kernel(1), 37, 53, 0.0, 0, DM.noise(37, 53), M.NORM_NONE)
    assert np.array_equal(zero_sigma, img)


@pytest.mark.parametrize("hw", [(37, 53), (53, 37), (41, 43)])
def test_output_shape_equals_input_shape_for_odd_sizes(hw):
    h, w = hw
    img = DM.image(h, w)
    lh, lw = DM.low_size(h, w, 2.3)
    out, mid = M.degrade_model(img, DM.kernel((41, 1.4, 1.4, 0.0, True)), lh, lw, 5.0, 60, DM.noise(lh, lw), M.NORM_MAX, with_jpeg=True)
    assert out.shape == img.shape and out.dtype == np.uint8 and mid.shape == (lh, lw, 3)
    assert out.max() == 255   # norm = max: the brightest value reaches white
    with pytest.raises(ValueError, match="too small"):
        M.degrade_model(img[:20], DM.kernel((41, 1.4, 1.4, 0.0, True)), 10, 10)


def test_blur_keeps_a_constant_image_and_reflects():
    flat = np.full((30, 25, 3), 77, dtype=np.uint8)
    x = M.blur(M.to_float(flat), DM.kernel((41, 10.0, 10.0, 0.0, True)))
    assert np.abs(x - np.float32(77 / 255)).max() < 1e-6
    ramp = np.tile(np.arange(30, dtype=np.uint8)[:, None, None] * 8, (1, 25, 3))
    k = np.zeros((5, 5))
    k[0, 2] = 1.0   # picks the pixel two rows up: row 0 reads row 2 (REFLECT_101), row 1 reads row 1
    y = M.blur(M.to_float(ramp), k)
    assert np.array_equal(y[0], M.to_float(ramp)[2]) and np.array_equal(y[1], M.to_float(ramp)[1]) and np.array_equal(y[5], M.to_float(ramp)[3])


# ---------------------------------------------------------------- ABI
def test_header_symbols_and_build_list_move_together():
    from instarevive_amd import _lib as L
    from instarevive_amd import build
    lib = L.load_library()
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "int ir_degrade(ir_ctx* ctx, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, const ir_degrade_params* params," in header
    assert "int ir_degrade_qtables(int q, uint16_t* luma64, uint16_t* chroma64);" in header and "IR_STAGE_DEGRADE = 16" in header
    assert {"ir_degrade", "ir_degrade_qtables"} <= set(L.SYMBOLS) and L.STAGE_DEGRADE == 16
    assert hasattr(lib, "ir_degrade") and hasattr(lib, "ir_degrade_qtables")
    assert lib.ir_abi_version() == 3   # the entry points are additive
    assert "degrade.hip" in build.SOURCES
    flags = build.FLAGS + build.FILE_FLAGS.get("degrade.hip", [])
    assert [f for f in flags if f.startswith("-ffp-contract")][-1] == "-ffp-contract=off"
    import ctypes as C
    assert C.sizeof(L.DegradeParams) == 40   # two pointers, five ints, one float


def test_workspace_needs_no_context_and_covers_the_planes():
    for h, w in ((48, 40), (256, 192), (2048, 2048)):
        need = D.ws_bytes(h, w)
        ph, pw = (h + 15) & ~15, (w + 15) & ~15
        assert need >= 2 * h * w * 12 + ph * pw * 3 // 2 and need % 256 == 0
        assert need <= 2 * h * w * 12 + ph * pw * 3 // 2 + 4 * ((h + 31) // 32) * ((w + 31) // 32) + 8 * 256
