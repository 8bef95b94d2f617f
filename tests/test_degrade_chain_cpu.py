"""The host side of --degrade realesrgan (instarevive_amd/degrade.py) and its definition (tools/degrade_folder.py:degrade_chain_model), without a GPU.

Every part of the model is held to something that is not the model: the filter and the three resizes to torch.nn.functional on the CPU, the
kernel builders, filter2D and the DiffJPEG pieces to the reference's own outputs (tests/golden/degrade_chain.npz, made by
make_degrade_chain_golden.py), the Poisson inversion to scipy.stats.poisson.ppf, the built-in recipe to the reference's yaml
(tests/golden/realesrgan_val.json).

The gate on a float comparison is |model - other| <= (T + 8) * 2^-24 * sum|weights| * max|x| with T the number of terms of the op's sum:
T * 2^-24 bounds the forward error of a float32 sum of T products in any order (the model's own fp64 sum adds nothing at that scale), and the
eight further units cover weights that the other side holds in float32 and the model in float64 or the other way round. It is derived, not tuned."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from instarevive_amd import _lib as L
from instarevive_amd import degrade as D
from tools import degrade_folder as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MODES = {"area": M.MODE_AREA, "bilinear": M.MODE_BILINEAR, "bicubic": M.MODE_BICUBIC}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "degrade_chain.npz"))


def _image(h, w, seed=0):
    return np.random.default_rng([h, w, seed]).random((h, w, 3), dtype=np.float32)


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]


def _hwc(t):
    return t[0].permute(1, 2, 0).numpy()


def test_constants_agree_between_the_model_the_binding_and_the_header():
    assert (M.OP_FILTER, M.OP_RESIZE, M.OP_GAUSS, M.OP_POISSON, M.OP_DIFFJPEG) == (L.CHAIN_FILTER, L.CHAIN_RESIZE, L.CHAIN_GAUSS, L.CHAIN_POISSON, L.CHAIN_DIFFJPEG)
    assert (M.MODE_AREA, M.MODE_BILINEAR, M.MODE_BICUBIC) == (L.CHAIN_AREA, L.CHAIN_BILINEAR, L.CHAIN_BICUBIC)
    assert (M.CHAIN_MAX_OPS, M.CHAIN_MAX_KSIZE) == (L.CHAIN_MAX_OPS, L.CHAIN_MAX_KSIZE) == (16, 21)
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "IR_STAGE_DEGRADE_CHAIN = 17" in header and "int ir_degrade_chain(ir_ctx* ctx, void* stream" in header
    assert "ir_degrade_chain" in L.SYMBOLS and L.STAGE_DEGRADE_CHAIN == 17
    assert hasattr(L.load_library(), "ir_degrade_chain")
    import ctypes as C
    assert C.sizeof(L.ChainOp) == 32 and C.sizeof(L.Chain) == 24 + 16 * 32
    tables = D.chain_tables()
    assert np.array_equal(tables[:9 * 256].reshape(9, 256), M.poisson_exp_table())
    assert np.array_equal(tables[9 * 256:9 * 256 + 4096].reshape(64, 64), M.dct_basis())
    assert np.array_equal(tables[-128:-64], M.DCT_SCALE.astype(np.float64)) and np.array_equal(tables[-64:], M.IDCT_ALPHA.astype(np.float64))
    assert all(float(D.jpeg_factor(q)) == float(M.jpeg_factor(q)) for q in (30.5, 49.9, 50.0, 95.0))


# ---------------------------------------------------------------- FILTER
def test_filter_against_torch_conv2d():
    """T = 441. The kernel is a generalized anisotropic one padded to 21, on 11 x 16 (the reflection reaches the whole image) and 33 x 70."""
    k = D.pad_kernel(D.generalized_gaussian(13, 2.5, 0.9, -1.1, 1.7, False))
    worst = 0.0
    for h, w in ((11, 16), (33, 70)):
        x = _image(h, w)
        pad = F.pad(_nchw(x), (10, 10, 10, 10), mode="reflect")
        ref = _hwc(F.conv2d(pad.view(3, 1, h + 20, w + 20), torch.from_numpy(k).float().view(1, 1, 21, 21)).view(1, 3, h, w))
        err = float(np.abs(M.blur(x, k) - ref).max())
        gate = (441 + 8) * U * np.abs(k).sum() * float(x.max())
        print(f"filter {h} x {w}: max |model - torch| {err:.3g}, gate {gate:.3g}")
        assert err <= gate
        worst = max(worst, err)
    assert worst > 0   # float32 and float64 sums do differ: the comparison is not vacuous


def test_filter_against_the_references_filter2d(golden):
    x, k = M.to_float(golden["filter_img"]), golden["kernel_2"]
    err = float(np.abs(M.blur(x, k) - golden["filter_out"]).max())
    gate = (441 + 8) * U * np.abs(k).sum() * float(x.max())
    print(f"filter2D 24 x 31: max |model - reference| {err:.3g}, gate {gate:.3g}")
    assert err <= gate
    with pytest.raises(ValueError, match="too small"):
        M.blur(_image(10, 30), k)


# ---------------------------------------------------------------- RESIZE
def _weight_sum(mode, src, dst, scale):
    """The largest sum of |weights| along one axis."""
    if mode != M.MODE_BICUBIC:
        return 1.0
    return float(np.abs(np.stack(M._cubic_taps(src, dst, scale)[1])).sum(axis=0).max())


SIZES = [((37, 53), (13, 19)), ((13, 19), (19, 28)), ((12, 16), (48, 64)), ((20, 30), (20, 30)), ((20, 30), (7, 50))]   # down, up, x 4, keep, mixed
FACTORS = [((37, 53), 0.37), ((13, 19), 1.5), ((20, 30), 0.37), ((20, 30), 1.0), ((64, 48), 0.15), ((31, 40), 1.37)]


@pytest.mark.parametrize("name", list(MODES))
def test_resize_against_torch_interpolate(name):
    """Both forms of the call: size= maps with in / out, scale_factor= with 1 / scale_factor (on 20 x 30 at 0.37 the two differ by 0.6 in value).
    T = 4, 16, or the window."""
    mode = MODES[name]
    for (h, w), (oh, ow) in SIZES:
        x = _image(h, w)
        ref = _hwc(F.interpolate(_nchw(x), size=(oh, ow), mode=name))
        got = M.resize(x, mode, oh, ow, 0.0)
        T = {M.MODE_BILINEAR: 4, M.MODE_BICUBIC: 16}.get(mode, (-(-h // oh) + 1) * (-(-w // ow) + 1))
        gate = (T + 8) * U * _weight_sum(mode, h, oh, 0.0) * _weight_sum(mode, w, ow, 0.0) * float(x.max())
        err = float(np.abs(got - ref).max())
        print(f"{name} size {h} x {w} -> {oh} x {ow}: max |model - torch| {err:.3g}, gate {gate:.3g}")
        assert got.shape == ref.shape and got.dtype == np.float32 and err <= gate
    for (h, w), s in FACTORS:
        x = _image(h, w)
        ref = _hwc(F.interpolate(_nchw(x), scale_factor=s, mode=name))
        oh, ow = ref.shape[:2]
        assert (oh, ow) == (int(np.floor(h * s)), int(np.floor(w * s)))
        got = M.resize(x, mode, oh, ow, s)
        T = {M.MODE_BILINEAR: 4, M.MODE_BICUBIC: 16}.get(mode, (-(-h // oh) + 1) * (-(-w // ow) + 1))
        gate = (T + 8) * U * _weight_sum(mode, h, oh, s) * _weight_sum(mode, w, ow, s) * float(x.max())
        err = float(np.abs(got - ref).max())
        print(f"{name} scale_factor {s} on {h} x {w}: max |model - torch| {err:.3g}, gate {gate:.3g}")
        assert err <= gate
    with pytest.raises(ValueError, match="floor"):
        M.resize(_image(20, 30), mode, 8, 11, 0.37)


def test_scale_factor_and_size_forms_differ():
    """The trap: at 0.37 on 20 x 30 the output is 7 x 11 either way, and the two coordinate rules give different images."""
    x = _image(20, 30)
    a, b = M.resize(x, M.MODE_BILINEAR, 7, 11, 0.37), M.resize(x, M.MODE_BILINEAR, 7, 11, 0.0)
    assert float(np.abs(a - b).max()) > 0.1


# ---------------------------------------------------------------- kernel builders, recipe
def test_kernel_builders_equal_the_references(golden):
    from tests.golden.make_degrade_chain_golden import KERNEL_CASES, SINC_CASES
    for i, (fam, K, sx, sy, th, beta, iso) in enumerate(KERNEL_CASES):
        got = {"gauss": lambda: D.bivariate_gaussian(K, sx, sy, th, iso), "generalized": lambda: D.generalized_gaussian(K, sx, sy, th, beta, iso),
               "plateau": lambda: D.plateau(K, sx, sy, th, beta, iso)}[fam]()
        assert got.dtype == np.float64 and np.allclose(got, golden[f"kernel_{i}"], rtol=1e-13, atol=0), (fam, K)
    for i, (cutoff, K, pad) in enumerate(SINC_CASES):
        got = D.circular_lowpass_kernel(cutoff, K, pad)
        assert got.shape == golden[f"sinc_{i}"].shape and np.allclose(got, golden[f"sinc_{i}"], rtol=1e-13, atol=1e-18), (cutoff, K)
    assert D.pad_kernel(np.ones((7, 7))).shape == (21, 21) and D.pad_kernel(np.ones((7, 7))).sum() == 49


def test_sinc_kernel_names_scipy_when_it_is_absent(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_scipy(name, *a, **kw):
        if name.split(".")[0] == "scipy":
            raise ImportError("No module named 'scipy'")
        return real(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(D.DegradeError, match="scipy"):
        D.circular_lowpass_kernel(1.3, 13)


def test_mixed_kernel_beta_rule():
    """A coin, then beta from [low, 1] or [1, high]: both halves occur, no beta leaves its range, every type is drawn."""
    rec = D.load_recipe("realesrgan")
    rng = np.random.default_rng(0)
    seen, low, high = set(), 0, 0
    for _ in range(400):
        k, info = D.mixed_kernel(rng, rec["kernel_list"], rec["kernel_prob"], 9, rec["blur_sigma"], rec["betag_range"], rec["betap_range"])
        seen.add(info["kind"])
        assert k.shape == (9, 9) and abs(k.sum() - 1) < 1e-12
        if "beta" in info:
            lo, hi = rec["betag_range"] if info["kind"].startswith("generalized") else rec["betap_range"]
            assert lo <= info["beta"] <= hi
            low, high = low + (info["beta"] < 1), high + (info["beta"] >= 1)
    assert seen == set(D.CHAIN_KERNELS) and low > 20 and high > 20


def test_builtin_recipe_equals_the_references_yaml(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "realesrgan_val.json")) as f:
        want = json.load(f)
    assert D.REALESRGAN_RECIPE == want and D.load_recipe("realesrgan") == want
    path = tmp_path / "mine.json"
    path.write_text(json.dumps({"chain": "realesrgan", "stage2_scale": 2, "final_sinc_prob": 0.0}))
    rec = D.load_recipe(str(path))
    assert rec["stage2_scale"] == 2 and rec["jpeg_range"] == [30, 95]
    assert D.load_recipe("lq") == D.LQ_RECIPE and "chain" not in D.load_recipe({"norm": "max"})   # the first-order recipe is as it was


# ---------------------------------------------------------------- DIFFJPEG
def _jpeg_case(golden, s, qi):
    from tests.golden.make_degrade_chain_golden import QUALITIES
    return M.to_float(golden[f"jpeg_img_{s}"]), QUALITIES[qi]


@pytest.mark.parametrize("s,qi", [(s, qi) for s in range(2) for qi in range(3)])
def test_diffjpeg_pieces_against_the_reference(golden, s, qi):
    """The quotients ahead of the rounding and the decompression of the model's own integers: T = 64."""
    x, q = _jpeg_case(golden, s, qi)
    h, w = x.shape[:2]
    f, basis = M.jpeg_factor(q), M.dct_basis()
    planes = M.jpeg_planes(x)
    coefs = []
    for c, (p, name) in enumerate(zip(planes, ("y", "cb", "cr"))):
        table = M.JPEG_TABLES[min(c, 1)].reshape(64) * np.float32(f)
        got = M.jpeg_quotients(p, M.JPEG_TABLES[min(c, 1)], f, basis)
        # the sum's weights: scale * basis / (table * factor) per frequency, on samples of at most 128 (the colour stage adds 3 + 8 units of 255)
        wsum = (np.abs(basis) * M.DCT_SCALE[None, :]).sum(axis=0) / table
        gate = ((64 + 8) * U * wsum * 128.0 + (3 + 8) * U * 255.0 * wsum)[None, :]
        err = np.abs(got - golden[f"jpeg_quot_{s}_{qi}_{name}"])
        print(f"{h} x {w} q {q} {name}: max |model - reference| quotient {err.max():.3g}, gate at that place {gate[0][err.max(axis=0).argmax()]:.3g}")
        assert np.all(err <= gate)
        coefs.append(np.rint(got))
    back = [M.jpeg_plane_back(cf, M.JPEG_TABLES[min(c, 1)], f, basis, *p.shape) for c, (cf, p) in enumerate(zip(coefs, planes))]
    got = M.jpeg_rgb(back[0], back[1], back[2], h, w)
    # per plane value: 64 terms of |coefficient * table * alpha| * 0.25 |basis| <= the block's own sum; then the 3-term matrix (weights sum <= 2.8) over 255
    mags = [np.abs(cf.astype(np.float64) * (M.JPEG_TABLES[min(c, 1)].reshape(64) * np.float32(f)) * M.IDCT_ALPHA).sum(axis=1).max() * 0.25 for c, cf in enumerate(coefs)]
    gate = ((64 + 8) * U * max(mags) * 2.8 + (3 + 8) * U * 2.8 * 255.0) / 255.0
    err = float(np.abs(got - golden[f"jpeg_dec_{s}_{qi}"]).max())
    print(f"{h} x {w} q {q}: max |model - reference| decompressed {err:.3g}, gate {gate:.3g}")
    assert err <= gate


@pytest.mark.parametrize("s,qi", [(s, qi) for s in range(2) for qi in range(3)])
def test_diffjpeg_round_trip_against_the_reference(golden, s, qi):
    """The whole module outside the blocks that hold a near-tie (under 5 % by the fixture generator's assertion): the decompression's gate."""
    x, q = _jpeg_case(golden, s, qi)
    h, w = x.shape[:2]
    got, ref, tie = M.diffjpeg(x, q), golden[f"jpeg_full_{s}_{qi}"], golden[f"jpeg_tie_{s}_{qi}"]
    assert tie.mean() < 0.05
    keep = ~np.repeat(np.repeat(tie, 8, axis=0), 8, axis=1)[:h, :w]
    gate = ((64 + 8) * U * 8 * 255.0 * 2.8 + (3 + 8) * U * 2.8 * 255.0) / 255.0   # |plane - 128| <= 8 * 255 bounds any block's coefficient sum
    err = float(np.abs(got - ref)[keep].max())
    print(f"{h} x {w} q {q}: max |model - reference| round trip {err:.3g} on {keep.mean() * 100:.0f} % of the pixels, gate {gate:.3g}")
    assert got.shape == ref.shape and got.dtype == np.float32 and err <= gate
    assert float(np.abs(got - x).max()) > 1e-3   # and the op does something


def test_jpeg_tables_are_the_transposed_ones():
    assert M.JPEG_TABLES[0][0, 1] == 12 and M.JPEG_TABLES[0][1, 0] == 11 and M.JPEG_TABLES[1][0, 3] == 47 and M.JPEG_TABLES[1][3, 3] == 99
    assert float(M.jpeg_factor(30.5)) == float(np.float32(5000.0) / np.float32(30.5) / np.float32(100.0))
    assert float(M.jpeg_factor(95.0)) == pytest.approx(0.1, rel=1e-6)


# ---------------------------------------------------------------- POISSON, GAUSS
def test_poisson_inversion_against_scipy():
    from scipy.stats import poisson
    lam = np.repeat(np.array([0.0, 0.004, 0.3, 1.0, 7.5, 64.0, 200.0, 256.0]), 2000)
    u = np.tile(np.concatenate([np.random.default_rng(5).random(1990), [0.0, 1e-300, 1e-9, 0.5, 0.999, 1 - 1e-9, 1 - 1e-12, 0.25, 0.75, 0.9]]), 8)
    k = M.poisson_invert(lam, np.exp(-lam), u)
    ref = poisson.ppf(u, lam)
    ks = np.arange(0, 600)[None, :]
    steps = np.concatenate([np.zeros((lam.size, 1)), poisson.cdf(ks, lam[:, None])], axis=1)   # F(-1) = 0 is a step too: scipy's ppf(0) is -1
    keep = np.abs(steps - u[:, None]).min(axis=1) > 1e-12   # leave out a u within 1e-12 of a step of the distribution
    assert keep.mean() > 0.99
    assert np.array_equal(k[keep], ref[keep].astype(np.int64)), np.argwhere(k[keep] != ref[keep])[:4]


@pytest.mark.parametrize("levels,vals", [(1, 1), (2, 2), (200, 256), (256, 256), (3, 4), (129, 256), (128, 128)])
def test_poisson_vals_rule(levels, vals):
    """2 ** ceil(log2(distinct levels)) on images with that many levels; the noise of a one-level image at lambda = r is still Poisson."""
    lv = np.resize(np.arange(levels), (16, 16, 3)).astype(np.int64)
    x = (lv.astype(np.float32) / np.float32(255.0))
    assert len(np.unique(M.levels_of(x))) == levels and M.poisson_vals(M.levels_of(x)) == vals == int(2 ** np.ceil(np.log2(levels)))
    u = np.random.default_rng(levels).random((16, 16, 3))
    out = M.poisson_noise(x, u, 1.0, False)
    k = M.poisson_invert((x * np.float32(vals)).astype(np.float64), M.poisson_exp_table()[int(np.log2(vals))][lv], u)
    assert np.array_equal(out, np.clip(x + (k.astype(np.float32) / np.float32(vals) - x), 0, 1).astype(np.float32))
    g = M.poisson_noise(x, u[..., 0], 0.5, True)
    assert g.shape == x.shape and g.dtype == np.float32 and float(g.min()) >= 0 and float(g.max()) <= 1


def test_exp_table_is_exp_of_the_float32_rate():
    t = M.poisson_exp_table()
    assert t.shape == (9, 256) and t.dtype == np.float64 and t[0, 0] == 1.0 and t[8, 255] == np.exp(-256.0)
    assert t[3, 100] == np.exp(-np.float64(np.float32(100) / np.float32(255) * np.float32(8)))


def test_gauss_gray_uses_one_field_for_three_channels():
    x = _image(9, 11)
    n = np.random.default_rng(1).standard_normal((9, 11), dtype=np.float32)
    got = M.gauss_noise(x, n, 12.5, True)
    assert np.array_equal(got, M.add_noise(x, np.repeat(n[..., None], 3, axis=2), 12.5))
    with pytest.raises(ValueError):
        M.gauss_noise(x, n, 12.5, False)


def test_finish_rounds_half_to_even():
    x = np.array([[[0.5 / 255, 1.5 / 255, 2.5 / 255]], [[-1.0, 2.0, 254.5 / 255]]], dtype=np.float64).astype(np.float32)
    x[0, 0] = np.array([0.5, 1.5, 2.5], dtype=np.float32) / np.float32(255.0)
    want = np.clip(torch.round(torch.from_numpy(x) * 255.0), 0, 255).numpy().astype(np.uint8)
    assert np.array_equal(M.finish(x), want)


# ---------------------------------------------------------------- draws, refusals
def test_draws_depend_on_the_file_alone_and_reach_every_op():
    rec = D.load_recipe("realesrgan")
    a = D.draw(rec, "sub/x.png", 96, 128, 7)
    assert isinstance(a, D.ChainParams) and D.draw_chain(rec, "sub\\x.png", 96, 128, 7).describe() == a.describe()
    for _ in range(2):   # whichever batch or worker meets the file, and whatever was drawn before it
        D.draw(rec, "other.png", 128, 96, 7)
        b = D.draw(rec, "sub/x.png", 96, 128, 7)
        assert len(a.ops) == len(b.ops) and all(np.array_equal(p, q) if isinstance(p, np.ndarray) else p == q for x, y in zip(a.ops, b.ops) for p, q in zip(x, y))
    assert D.draw(rec, "sub/x.png", 96, 128, 8).describe() != a.describe()
    kinds, modes, orders, gray, pulse, first_forms, blur2 = set(), set(), set(), set(), set(), set(), set()
    for i in range(200):
        try:
            p = D.draw(rec, f"f{i}.png", 128, 160, 1)
        except D.DegradeError as e:
            assert "too small" in str(e)
            continue
        assert len(p.ops) <= L.CHAIN_MAX_OPS and p.ops[0][0] == L.CHAIN_FILTER and p.ops[1][0] == L.CHAIN_RESIZE and p.ops[1][4] > 0
        assert p.ops[-1] == (L.CHAIN_RESIZE, L.CHAIN_BICUBIC, 128, 160, 0.0) and D.check_chain(p, 128, 160)[0] >= 128
        first_forms.add("up" if p.ops[1][4] > 1 else ("down" if p.ops[1][4] < 1 else "keep"))
        for op in p.ops:
            kinds.add(op[0])
            if op[0] == L.CHAIN_RESIZE:
                modes.add(op[1])
            if op[0] in (L.CHAIN_GAUSS, L.CHAIN_POISSON):
                gray.add((op[0], bool(op[3])))
            if op[0] == L.CHAIN_DIFFJPEG:
                assert 30 <= op[1] <= 95 and op[1] != int(op[1])
        orders.add(p.info["back_first"])
        pulse.add(p.info["final_sinc"]["kind"])
        blur2.add(sum(op[0] == L.CHAIN_FILTER for op in p.ops))
        assert [op[0] for op in p.ops].index(L.CHAIN_DIFFJPEG) == 3
    assert kinds == {1, 2, 3, 4, 5} and modes == {0, 1, 2} and orders == {True, False} and pulse == {"sinc", "pulse"}
    assert gray == {(L.CHAIN_GAUSS, False), (L.CHAIN_GAUSS, True), (L.CHAIN_POISSON, False), (L.CHAIN_POISSON, True)}
    assert first_forms == {"up", "down", "keep"} and blur2 >= {1, 2, 3}


def test_model_runs_a_drawn_chain_and_taps_every_op():
    rec = D.load_recipe("realesrgan")
    img = np.random.default_rng(3).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    p = next(D.draw(rec, f"t{i}.png", 48, 64, 3) for i in range(50) if _draws(rec, f"t{i}.png", 48, 64, 3))
    out = M.degrade_chain_model(img, p.ops)
    assert out.shape == img.shape and out.dtype == np.uint8 and not np.array_equal(out, img)
    for t in range(len(p.ops)):
        again, tap = M.degrade_chain_model(img, p.ops, tap=t)
        assert np.array_equal(again, out) and tap.dtype == np.float32 and tap.shape == D.tap_shape(p, 48, 64, t)
    assert np.array_equal(M.degrade_chain_model(img, ()), img)   # float32(v / 255) * 255 rounds back to v


def _draws(rec, name, h, w, seed):
    try:
        D.draw(rec, name, h, w, seed)
        return True
    except D.DegradeError:
        return False


def test_refusals():
    rec = D.load_recipe("realesrgan")
    for h, w in ((43, 64), (64, 43), (40, 40)):
        with pytest.raises(D.DegradeError, match="too small"):   # stage2_scale 4: the final sinc, or a blur before it, would meet a side below 11
            D.draw_chain({**rec, "final_sinc_prob": 1.0}, "a.png", h, w, 1)
    assert any(_draws(rec, f"s{i}.png", 44, 44, 1) for i in range(40))   # 44 is the least side the recipe can take
    for flag in ("use_sharpener", "resize_hq"):
        with pytest.raises(D.DegradeError, match=flag):
            D.load_recipe({"chain": "realesrgan", flag: True})
    with pytest.raises(D.DegradeError, match="unknown chain"):
        D.load_recipe({"chain": "bsrgan"})
    with pytest.raises(D.DegradeError, match="unknown keys"):
        D.load_recipe({"chain": "realesrgan", "downsample_range": [2, 4]})
    with pytest.raises(D.DegradeError, match="skew"):
        D.load_recipe({"chain": "realesrgan", "kernel_list": ["skew"], "kernel_prob": [1]})
    with pytest.raises(D.DegradeError, match="plateau_iso"):   # the first-order recipe still refuses the second-order kernels by name
        D.load_recipe({"kernel_list": ["plateau_iso"], "kernel_prob": [1]})
    k = D.delta_kernel(21)
    good = D.ChainParams(((L.CHAIN_FILTER, k), (L.CHAIN_RESIZE, L.CHAIN_AREA, 24, 32, 0.5), (L.CHAIN_RESIZE, L.CHAIN_BICUBIC, 48, 64, 0.0)))
    assert D.check_chain(good, 48, 64) == (48, 64)
    bad = {
        "unknown resize mode": ((L.CHAIN_RESIZE, 3, 48, 64, 0.0),), "floor": ((L.CHAIN_RESIZE, 0, 25, 32, 0.5), (L.CHAIN_RESIZE, 0, 48, 64, 0.0)),
        "ends at": ((L.CHAIN_RESIZE, 0, 24, 32, 0.0),), "too small": ((L.CHAIN_RESIZE, 0, 10, 64, 0.0), (L.CHAIN_FILTER, k), (L.CHAIN_RESIZE, 0, 48, 64, 0.0)),
        "unknown kind": ((9,),), "quality": ((L.CHAIN_DIFFJPEG, 0.5),), "at most 16": ((L.CHAIN_DIFFJPEG, 50.5),) * 17,
        "field": ((L.CHAIN_GAUSS, np.zeros((48, 64), dtype=np.float32), 1.0, False),), "float64": ((L.CHAIN_POISSON, np.zeros((48, 64, 3), dtype=np.float32), 1.0, False),),
        "odd": ((L.CHAIN_FILTER, np.zeros((23, 23))),),
    }
    for match, ops in bad.items():
        with pytest.raises(D.DegradeError, match=match):
            D.check_chain(D.ChainParams(ops), 48, 64)
    with pytest.raises(ValueError):
        M.degrade_chain_model(np.zeros((48, 64, 3), dtype=np.uint8), ((M.OP_RESIZE, 3, 48, 64, 0.0),))


def test_library_sizes_the_workspace_from_the_largest_intermediate():
    lib = L.load_library()
    a = lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 1, 64, 48, 64, 48, 0)
    b = lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 1, 64, 48, 96, 72, 0)
    assert 0 < a < b == lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 3, 64, 48, 96, 72, 0) == D.chain_ws_bytes(64, 48, 96, 72)
    assert a == lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 1, 64, 48, 0, 0, 0)   # nothing larger than the image itself
    assert lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 0, 64, 48, 64, 48, 0) == 0
    assert lib.ir_workspace_bytes(None, L.STAGE_DEGRADE_CHAIN, 1, 64, 9000, 64, 48, 0) == 0
