"""NIQE without a GPU: the definition's constants, the library's window, the host part of instarevive_amd.niqe against the model
(tools/evaluate_niqe.py), the parameter files, the ABI's refusals, the report's columns and the command lines' flag - and the planted bugs that
show that the gates of tests/test_niqe_gpu.py tell a kernel with another order of operations from the model."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from tests.support import niqe_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EN = NM.EN


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


# ---------------------------------------------------------------------------------------------------------------- the definition's constants
def test_resize_weights_are_the_eight_dyadic_values():
    w = EN.HALF_WEIGHTS
    assert [int(v * 256) for v in w] == [-3, -9, 29, 111, 111, 29, -9, -3] and all(v * 256 == int(v * 256) for v in w)
    total = 0.0
    for v in w:
        total += float(v)
    assert total == 1.0 and float(w.sum()) == 1.0
    # MATLAB's antialiased bicubic at scale 0.5: the cubic kernel (a = -0.5) stretched by 2, sampled at (t - 3.5) / 2, times 1 / 2
    x = np.abs((np.arange(8) - 3.5) / 2.0)
    cubic = np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x < 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0)) / 2.0
    assert np.array_equal(cubic / cubic.sum(), w)


def test_r_gam_is_strictly_increasing():
    from instarevive_amd import niqe
    for gam, r in (EN.gam_table(), niqe.gam_tables()):
        assert len(gam) == 9801 and gam[0] == 0.2 and abs(gam[-1] - 10.0) < 1e-9
        assert np.all(np.diff(r) > 0) and np.diff(r).min() > 1.6e-6
    assert np.allclose(EN.gam_table()[1], niqe.gam_tables()[1], rtol=1e-14, atol=0)


def test_library_window_is_the_formula():
    from instarevive_amd import niqe
    k = niqe.window()
    f = EN.window_formula()
    assert k.shape == (7, 7) and np.all(k > 0)
    assert np.all(np.abs(k - f) <= np.spacing(f))                           # within 1 ulp
    assert abs(math.fsum(k.reshape(-1).tolist()) - 1.0) <= 2.0 ** -52
    assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1, ::-1])
    assert np.array_equal(EN.window(), k)                                   # the model multiplies by the library's bits
    assert _library()[1].ir_niqe_window(None) == -1


def test_header_symbols_and_build_list_move_together():
    L, lib = _library()
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "int ir_niqe_stats(ir_ctx* ctx, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* out, void* ws," in header
    assert "int ir_niqe_window(double* k49);" in header and "IR_STAGE_NIQE = 14" in header
    assert {"ir_niqe_stats", "ir_niqe_window"} <= set(L.SYMBOLS) and L.STAGE_NIQE == 14
    assert hasattr(lib, "ir_niqe_stats") and hasattr(lib, "ir_niqe_window")
    assert lib.ir_abi_version() == 3   # the entry points are additive
    from instarevive_amd import build
    assert "niqe.hip" in build.SOURCES
    # the order of operations is part of the definition: -ffp-contract=fast fuses in the backend whatever the file's pragma says
    flags = build.FLAGS + build.FILE_FLAGS.get("niqe.hip", [])
    assert [f for f in flags if f.startswith("-ffp-contract")][-1] == "-ffp-contract=off"


def test_workspace_needs_no_context():
    L, lib = _library()
    from instarevive_amd import niqe
    ws = lambda n, h, w: lib.ir_workspace_bytes(None, L.STAGE_NIQE, n, h, w, 0, 0, 0)
    assert ws(1, 96, 96) >= 48 * 48 * 8 and ws(1, 2048, 2048) >= 1008 * 1008 * 8 and ws(1, 2048, 2048) < 1024 * 1024 * 8 + 256
    assert ws(1, 200, 300) == ws(1, 192, 288)                # the scored rectangle alone
    assert ws(3, 192, 288) >= 3 * 96 * 144 * 8
    assert ws(0, 96, 96) == 0 and ws(1, 95, 200) == 0 and ws(1, 200, 95) == 0 and ws(-1, 96, 96) == 0
    assert niqe.ws_bytes(2, 192, 96) == ws(2, 192, 96) and niqe.blocks_of(200, 300) == 6


def test_call_refuses_a_null_context_and_bad_sizes():
    _, lib = _library()
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is launched
    call = lambda img, out, ws, n, h, w, rows=192, pitch=576, wsb=1 << 24: lib.ir_niqe_stats(None, None, img, rows, pitch, n, h, w, out, ws, wsb)
    assert call(fake, fake, fake, 1, 192, 192) == -1        # the null context
    for n, h, w in [(0, 192, 192), (1, 95, 192), (1, 192, 95), (1, 193, 192), (1, 192, 193)]:
        assert call(fake, fake, fake, n, h, w) == -1, (n, h, w)
    assert call(None, fake, fake, 1, 192, 192) == -1 and call(fake, None, fake, 1, 192, 192) == -1 and call(fake, fake, None, 1, 192, 192) == -1
    assert call(fake, fake, fake, 1, 192, 192, wsb=0) == -1


# ---------------------------------------------------------------------------------------------------------------- the host part
@pytest.mark.parametrize("name", list(NM.cases()))
def test_features_and_score_from_the_models_statistics(name):
    from instarevive_amd import niqe
    stats, feat, score = NM.model(name)
    got = niqe.features_from_stats(stats)
    assert got.shape == feat.shape == (stats.shape[1], 36)
    assert np.array_equal(np.isnan(got), np.isnan(feat))
    ok = ~np.isnan(feat)
    assert np.all(np.abs(got[ok] - feat[ok]) <= 1e-12 * np.abs(feat[ok]))
    if score is None:
        with pytest.raises(niqe.NiqeError, match="two complete feature rows"):
            niqe.score(got, NM.params())
    else:
        assert abs(niqe.score(got, NM.params()) - score) <= 1e-12 * score


def test_nan_rows_are_handled_as_defined():
    from instarevive_amd import niqe
    stats, feat, score = NM.model("zero_block_480x672")
    nan_rows = np.isnan(feat).any(axis=1)
    assert int(nan_rows.sum()) == 1 and nan_rows[1 * 7 + 2]               # the all-zero block, and no other
    assert score is not None and np.isfinite(score)
    assert np.all(NM.alphas(feat)[nan_rows][:, :5] == 0.2)                # scale 1 (scale 2 rings at the block's edge): argmin over NaN distances is entry 0
    # the NaN row counts in the column means where it has a value (alpha) and in no covariance
    without = np.delete(feat, 1 * 7 + 2, axis=0)
    assert abs(EN.score_features(without, *NM.params()) - score) > 1e-6 * score
    # one complete row: no score
    img = NM.zero_block(192, 288, 8, block=(0, 0))[:96, :192]
    two = EN.image_stats(img)
    f2 = niqe.features_from_stats(two)
    assert int(np.isnan(f2).any(axis=1).sum()) == 1
    with pytest.raises(niqe.NiqeError):
        niqe.score(f2, NM.params())
    with pytest.raises(ValueError):
        EN.score_features(EN.block_features(two), *NM.params())
    assert math.isnan(niqe.score_or_nan(two, NM.params()))


def test_load_params_round_trips_mat_and_npz(tmp_path):
    from scipy.io import savemat
    from instarevive_amd import niqe
    mu, cov = NM.params()
    savemat(str(tmp_path / "p.mat"), {"mu_prisparam": mu.reshape(1, 36), "cov_prisparam": cov})
    np.savez(tmp_path / "p.npz", mu_prisparam=mu, cov_prisparam=cov)
    for name in ("p.mat", "p.npz"):
        m, c = niqe.load_params(str(tmp_path / name))
        assert m.shape == (36,) and c.shape == (36, 36) and np.array_equal(m, mu) and np.array_equal(c, cov)
        m2, c2 = EN.load_params(str(tmp_path / name))
        assert np.array_equal(m2, mu) and np.array_equal(c2, cov)
    np.savez(tmp_path / "short.npz", mu_prisparam=mu[:35], cov_prisparam=cov)
    np.savez(tmp_path / "flat.npz", mu_prisparam=mu, cov_prisparam=cov.reshape(-1))
    np.savez(tmp_path / "other.npz", mu=mu, cov=cov)
    savemat(str(tmp_path / "wrong.mat"), {"mu_prisparam": mu, "cov_prisparam": cov[:35]})
    (tmp_path / "text.mat").write_text("not a mat file")
    for name in ("short.npz", "flat.npz", "other.npz", "wrong.mat", "text.mat", "missing.npz"):
        with pytest.raises(niqe.NiqeError, match=name.replace(".", r"\.")):
            niqe.load_params(str(tmp_path / name))


def test_report_writes_the_new_columns_and_still_the_old(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    alone = Report(str(tmp_path / "n.csv"), niqe=True, paired=False)
    alone.add("b.png", niqe=5.25)
    alone.add_scores("a,x.png", (4.123456789012345,))
    assert alone.write() == ["niqe: 4.68673"]
    assert (tmp_path / "n.csv").read_text().splitlines()[0] == "file,niqe"
    assert read_report(str(tmp_path / "n.csv")) == {"b.png": (5.25,), "a,x.png": (4.123456789012345,)}
    both = Report(str(tmp_path / "b.csv"), lpips=True, niqe=True)
    both.add_scores("a.png", (30.5, 0.9, 0.25, 6.5))
    both.add("b.png", 31.5, 0.8, 0.75, niqe=7.5)
    assert both.write() == ["psnr: 31.00000", "ssim: 0.85000", "lpips: 0.50000", "niqe: 7.00000"]
    assert (tmp_path / "b.csv").read_text().splitlines()[0] == "file,psnr_y,ssim_y,lpips,niqe"
    assert read_report(str(tmp_path / "b.csv")) == {"a.png": (30.5, 0.9, 0.25, 6.5), "b.png": (31.5, 0.8, 0.75, 7.5)}
    three = Report(str(tmp_path / "t.csv"), niqe=True)
    three.add_scores("a.png", (30.5, 0.9, 6.5))
    assert three.write() == ["psnr: 30.50000", "ssim: 0.90000", "niqe: 6.50000"]
    assert (tmp_path / "t.csv").read_text().splitlines()[0] == "file,psnr_y,ssim_y,niqe"
    old = Report(str(tmp_path / "o.csv"))
    old.add("a.png", 30.5, 0.9)
    assert old.write() == ["psnr: 30.50000", "ssim: 0.90000"] and (tmp_path / "o.csv").read_text() == "file,psnr_y,ssim_y\na.png,30.5,0.9\n"
    assert old.rows == [("a.png", 30.5, 0.9)]
    for bad in (lambda: old.add("x", 1.0, 1.0, niqe=1.0), lambda: alone.add("x", 1.0, 1.0, niqe=1.0), lambda: three.add("x", 1.0, 1.0),
                lambda: three.add_scores("x", (1.0, 1.0)), lambda: Report(paired=False)):
        with pytest.raises(MetricsError):
            bad()


def test_command_lines_parse_and_refuse_a_missing_parameter_file(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    assert inf.parse_args().niqe_params is None and eval_batch.parse_args().niqe_params is None
    assert inf.load_niqe_params(inf.parse_args()) is None
    missing = str(tmp_path / "nowhere.mat")
    monkeypatch.setattr(sys, "argv", base + ["--niqe_params", missing])
    assert inf.parse_args().niqe_params == missing and eval_batch.parse_args().niqe_params == missing
    # refused before any model is touched: neither the device check nor the loaders run
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match="nowhere.mat"):
            main()
    assert touched == []
    np.savez(tmp_path / "bad.npz", mu_prisparam=np.zeros(3), cov_prisparam=np.zeros((36, 36)))
    monkeypatch.setattr(sys, "argv", base + ["--niqe_params", str(tmp_path / "bad.npz")])
    with pytest.raises(SystemExit, match="bad.npz"):
        inf.main()
    mu, cov = NM.params()
    np.savez(tmp_path / "good.npz", mu_prisparam=mu, cov_prisparam=cov)
    monkeypatch.setattr(sys, "argv", base + ["--niqe_params", str(tmp_path / "good.npz")])
    got = inf.load_niqe_params(inf.parse_args())
    assert np.array_equal(got[0], mu) and np.array_equal(got[1], cov)
    monkeypatch.setattr(sys, "argv", ["evaluate_niqe.py", "-i", "a", "--niqe_params", "p.npz", "--backend", "gpu", "--ntest", "3"])
    seen = {}
    monkeypatch.setattr(EN, "evaluate", lambda *a, **k: seen.update(k, args=a))
    EN.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "p.npz", 3)


def test_evaluate_niqe_averages_a_folder(tmp_path):
    from PIL import Image
    mu, cov = NM.params()
    np.savez(tmp_path / "p.npz", mu_prisparam=mu, cov_prisparam=cov)
    for name in ("ramp_96x192", "smooth_288x96", "noise_96x96"):
        Image.fromarray(NM.cases()[name]).save(tmp_path / f"{name}.png")
    lines = []
    avg = EN.evaluate(str(tmp_path), str(tmp_path / "p.npz"), log=lines.append)
    want = (NM.model("ramp_96x192")[2] + NM.model("smooth_288x96")[2]) / 2
    assert abs(avg - want) <= 1e-12 * want and lines[-1] == f"niqe: {want:.5f}" and "1 not scored" in lines[-2]


# ---------------------------------------------------------------------------------------------------------------- planted bugs
def _misses_the_gpu_gates(name, score=True, **variant):
    """A variant of the model on a case: (counts differ, largest relative deviation of the sums, relative change of the score or None)."""
    img = NM.cases()[name]
    stats, _, base = NM.model(name)
    st = EN.image_stats(img, **variant)
    counts, sums = NM.compare_stats(st, stats)
    rel = abs(EN.score_features(EN.block_features(st), *NM.params()) - base) / base if score else None
    print(f"{name} {variant}: counts differ {not counts}, sums by {sums:.3e}" + (f", score by {rel:.3e}" if score else ""))
    return not counts, sums, rel


def test_planted_separable_filter_flips_the_flat_patches():
    """A 7 + 7 sum in place of the 49-tap sum: the same filter up to rounding (sums within 1e-12), yet on the flat patches every sign of y - mu
    hangs on that rounding - the counts change, and the score by far more than the GPU gate."""
    differ, sums, rel = _misses_the_gpu_gates("patches_192x288", separable=True)
    assert differ and sums < NM.SUM_RTOL and rel > 1000 * NM.SCORE_RTOL
    # on an image without flat areas the two orders pass every gate: this is what makes the order invisible on ordinary test images
    differ, sums, rel = _misses_the_gpu_gates("smooth_288x96", separable=True)
    assert not differ and sums < NM.SUM_RTOL and rel < NM.SCORE_RTOL


def test_planted_non_circular_roll():
    differ, sums, rel = _misses_the_gpu_gates("patches_192x288", circular=False)
    assert differ and sums > NM.SUM_RTOL and rel > NM.SCORE_RTOL


def test_planted_wrong_diagonal():
    differ, sums, rel = _misses_the_gpu_gates("patches_192x288", shifts=((0, 1), (1, 0), (1, 1), (1, 1)))
    assert differ and sums > NM.SUM_RTOL and rel > NM.SCORE_RTOL


def test_planted_zero_padding():
    differ, sums, rel = _misses_the_gpu_gates("patches_192x288", mscn_pad="zero")
    assert differ and sums > NM.SUM_RTOL and rel > NM.SCORE_RTOL


def test_planted_resize_without_the_mirrored_border():
    differ, sums, rel = _misses_the_gpu_gates("patches_192x288", pad_mode="edge")
    assert sums > NM.SUM_RTOL and rel > NM.SCORE_RTOL
    st = EN.image_stats(NM.cases()["patches_192x288"], pad_mode="edge")
    assert np.array_equal(st[0], NM.model("patches_192x288")[0][0])       # scale 1 does not pass through the resize


def test_planted_biased_covariance():
    name = "patches_192x288"
    _, feat, base = NM.model(name)
    assert abs(EN.score_features(feat, *NM.params(), biased=True) - base) > NM.SCORE_RTOL * base


def test_planted_columns_after_rows_on_the_grey_ramp():
    """The half-size filter along the rows first: the same plane up to rounding. On the grey ramp with its flat 77 band, where 77 / 255 does not
    pass the filter exactly and y2 - mu is rounding noise everywhere, the counts of scale 2 change; scale 1 does not pass through the resize."""
    name = "gray_ramp_96x192"
    stats = NM.model(name)[0]
    st = EN.image_stats(NM.cases()[name], columns_first=False)
    assert np.array_equal(st[0], stats[0])
    counts, sums = NM.compare_stats(st[1], stats[1])
    assert not counts and sums < NM.SUM_RTOL
    unit = 77 / 255.0
    once = EN.half(np.full((96, 96), unit))
    assert once[5, 5] != unit                                             # `half` is inexact on a flat 77


def test_alpha_cannot_flip_on_rounding_for_any_gpu_input():
    """Every rn of every GPU test input lies at least 1e-9 (relative) from every midpoint of neighbouring r_gam entries: the device's statistics,
    within 1e-10 of the model's, select the same alpha."""
    for name in NM.cases():
        margin = NM.rn_margin(NM.model(name)[0])
        print(f"{name}: closest midpoint at {margin:.3e} relative")
        assert margin >= NM.MIDPOINT_RTOL, name
