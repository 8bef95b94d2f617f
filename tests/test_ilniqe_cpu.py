"""IL-NIQE without a GPU: the model (tools/evaluate_ilniqe.py) against independent forms, the noise floor that the gates of
tests/test_ilniqe_gpu.py are derived from (tests/support/ilniqe_cases.py), and the host code - the template files, the library's resize tables and
refusals, the report's column and the command lines' flag.

The floors measured here (scipy.fft against the dense DFT product in the kernel's k order, largest over the five cases): AGGD sums 1.1e-16,
mean / variance 0 (planes 4-6 pass through no transform), Weibull (k, lambda) 5.11e-14, score 1.72e-15, alpha cells that move by one step 0
of 29880; the transform itself 1.46e-15."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from tests.support import ilniqe_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EI = IC.EI


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


# ---------------------------------------------------------------------------------------------------------------- the model against independent forms
def test_resize_weights_sum_to_one_and_the_exact_half_is_niqes_table():
    for n_in in (24, 40, 524, 600, 700, 1048, 1100):
        idx, w = EI.resize_weights(n_in, 524)
        assert idx.shape == w.shape == (524, math.ceil(max(4.0, 4.0 * n_in / 524)) + 2)
        assert idx.min() >= 0 and idx.max() < n_in
        assert np.abs(np.array([math.fsum(r) for r in w.tolist()]) - 1.0).max() <= 2.0 ** -51
    idx, w = EI.resize_weights(1048, 524)
    assert np.array_equal(w * 256.0, np.tile([0.0, -3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0, 0.0], (524, 1)))
    assert np.array_equal(idx[5], np.arange(6, 16)) and np.array_equal(idx[0], [3, 2, 1, 0, 0, 1, 2, 3, 4, 5])      # inputs 2o - 3 .. 2o + 4, symmetric
    idx, w = EI.resize_weights(524, 524)                                                                              # the identity
    assert all(w[o][idx[o] == o].sum() == 1.0 and np.count_nonzero(w[o]) == 1 for o in (0, 1, 200, 523))


def test_a_constant_image_resizes_to_the_same_constant():
    for h, w in ((24, 24), (40, 700), (600, 1100)):
        out = EI.resize524(np.full((h, w, 3), 201, np.uint8))
        assert out.shape == (504, 504, 3) and np.abs(out - 201.0).max() <= 201.0 * 2.0 ** -50


def test_library_plan_holds_the_models_bits():
    """ir_ilniqe_plan (host only) against the model's tables for every case's size, bit for bit; its refusals."""
    from instarevive_amd import ilniqe
    _, lib = _library()
    for h, w in IC.SIZES.values():
        (i0, w0), (i1, w1) = ilniqe.plan_arrays(h, w)
        a0, b0 = EI.resize_weights(h, 524)
        a1, b1 = EI.resize_weights(w, 524)
        assert np.array_equal(i0, a0) and np.array_equal(i1, a1) and np.array_equal(w0.view(np.uint64), b0.view(np.uint64)) and np.array_equal(w1.view(np.uint64), b1.view(np.uint64))
        assert ilniqe.taps_of(h) == b0.shape[1] and ilniqe.taps_of(w) == b1.shape[1]
    n = lib.ir_ilniqe_plan_bytes(600, 1100)
    buf = np.zeros(n // 8 + 2, np.float64)
    assert n == 524 * (7 + 11) * 12 and lib.ir_ilniqe_plan_bytes(1, 50) == -1 and lib.ir_ilniqe_plan_bytes(50, 1) == -1
    assert lib.ir_ilniqe_plan(600, 1100, None, n) == -1 and lib.ir_ilniqe_plan(600, 1100, C.c_void_p(buf.ctypes.data), n - 1) == -1
    assert lib.ir_ilniqe_plan(600, 1100, C.c_void_p(buf.ctypes.data + 4), n) == -1 and lib.ir_ilniqe_plan(600, 1100, C.c_void_p(buf.ctypes.data), n) == 0


def test_package_tables_hold_the_models_bits():
    from instarevive_amd import ilniqe
    t = ilniqe.tables()
    assert np.array_equal(t["ilniqe.win5"], EI.gaussian_window(5, 5.0 / 6.0)) and np.array_equal(t["ilniqe.win6"], EI.gaussian_window(6, 0.9))
    for s in (1, 2):
        xg, g = EI.derivative_taps(s)
        assert len(g) == 11 and np.array_equal(t["ilniqe.taps"][s - 1], np.stack([xg, g]))
    assert np.array_equal(t["ilniqe.bank504"], EI.log_gabor_bank(504, 1)) and np.array_equal(t["ilniqe.bank252"], EI.log_gabor_bank(252, 2))
    for k in (t["ilniqe.win5"], t["ilniqe.win6"]):
        assert abs(math.fsum(k.reshape(-1).tolist()) - 1.0) <= 2.0 ** -51 and np.array_equal(k, k.T)


def test_log_gabor_bank_is_zero_at_dc_and_splits_into_even_and_odd_parts():
    """Every filter is real and zero at DC. Its even part F(u) + F(-u) carries the real part of a real image's response and its odd part the
    imaginary part: that is where conjugate symmetry must hold."""
    import scipy.fft
    rng = np.random.default_rng(3)
    for n, s in ((252, 2), (504, 1)):
        bank = EI.log_gabor_bank(n, s)
        assert bank.shape == (12, n, n) and np.all(bank[:, 0, 0] == 0.0) and np.all(bank >= 0.0) and bank.max() <= 1.0
        x = scipy.fft.fft2(rng.standard_normal((n, n)))
        for f in (0, 5, 11):
            flip = np.roll(bank[f][::-1, ::-1], (1, 1), (0, 1))                  # F(-u)
            resp = scipy.fft.ifft2(bank[f] * x)
            even, odd = scipy.fft.ifft2((bank[f] + flip) / 2.0 * x), scipy.fft.ifft2((bank[f] - flip) / 2.0 * x)
            scale = np.abs(resp).max()
            assert np.abs(even.imag).max() <= 1e-13 * scale and np.abs(odd.real).max() <= 1e-13 * scale
            assert np.abs(resp.real - even.real).max() <= 1e-13 * scale and np.abs(resp.imag - odd.imag).max() <= 1e-13 * scale
    # scale-major, orientation-minor: filters 0-3 share the first wavelength and peak at the same radius
    bank = EI.log_gabor_bank(252, 2)
    radius = lambda f: np.hypot(*[np.minimum(v, 252 - v) for v in np.unravel_index(np.argmax(bank[f]), (252, 252))])
    assert abs(radius(0) - radius(3)) <= 1.5 and radius(4) < radius(0) and radius(8) < radius(4)


def test_transforms_against_the_explicit_dft_matrix():
    import scipy.fft
    rng = np.random.default_rng(4)
    n = 252
    z = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    w = np.exp(-2j * np.pi * np.outer(np.arange(n), np.arange(n)) / n)
    ref_f, ref_i = w @ z @ w, np.conj(w) @ z @ np.conj(w) / (n * n)
    for fn in (EI.dft2_scipy, EI.dft2_dense):
        fr, fi = fn(z.real, z.imag, False)
        ir, ii = fn(z.real, z.imag, True)
        assert np.abs(fr + 1j * fi - ref_f).max() <= 1e-11 * np.abs(ref_f).max() and np.abs(ir + 1j * ii - ref_i).max() <= 1e-11 * np.abs(ref_i).max()
    assert np.abs(scipy.fft.ifft2(z) - ref_i).max() <= 1e-11 * np.abs(ref_i).max()
    c, s = EI.twiddles(n)
    assert np.array_equal(c, c.T) and c[0].tolist() == [1.0] * n and s[0].tolist() == [0.0] * n and c[1, 63] == math.cos(2.0 * math.pi * 63 / n)
    assert c[5, 101] == c[1, (5 * 101) % n]                                      # jk is reduced mod N first


def test_dft_floor():
    """The floor of ir_op_dft2_f64's comparison: the dense product in the kernel's k order against scipy.fft on the seeded input of the GPU test."""
    worst = 0.0
    for n in (252, 504):
        re, im = IC.dft_input(n)
        for inv in (False, True):
            s, d = EI.dft2_scipy(re, im, inv), EI.dft2_dense(re, im, inv)
            worst = max(worst, max(np.abs(s[0] - d[0]).max(), np.abs(s[1] - d[1]).max()) / np.abs(s[0] + 1j * s[1]).max())
    print(f"dense against scipy.fft: {worst:.3e} (recorded {IC.DFT_FLOOR:.3e})")
    assert 0.5 * IC.DFT_FLOOR <= worst <= IC.DFT_FLOOR


def test_weibull_fit_recovers_the_parameters_and_agrees_with_scipy():
    from scipy.stats import weibull_min
    rng = np.random.default_rng(6)
    truth = [(0.7, 2.0), (1.5, 0.3), (3.0, 40.0)]
    x = np.stack([lam * rng.weibull(k, 7056) for k, lam in truth])
    k, lam, steps = EI.weibull_fit(x, steps=True)
    assert steps.max() <= 10
    for i, (k0, l0) in enumerate(truth):
        # the asymptotic deviations of the maximum-likelihood estimates: 0.78 k / sqrt n and 1.053 (lambda / k) / sqrt n; four of them
        assert abs(k[i] - k0) <= 4 * 0.78 * k0 / math.sqrt(7056) and abs(lam[i] - l0) <= 4 * 1.053 * l0 / k0 / math.sqrt(7056)
        c, _, sc = weibull_min.fit(x[i], floc=0)
        assert abs(k[i] - c) <= 1e-2 and abs(lam[i] - sc) <= 1e-2 * sc           # its own stopping rule
    f = lambda kk, row: (row ** kk * np.log(row)).sum() / (row ** kk).sum() - np.log(row).mean() - 1.0 / kk
    assert all(abs(f(k[i], x[i])) < abs(f(k[i] + 0.02, x[i])) for i in range(3))
    # the rows of the GPU test take the step counts their names say
    rows = IC.weibull_rows()
    _, _, steps = EI.weibull_fit(np.stack(list(rows.values())), steps=True)
    taken = dict(zip(rows, steps.tolist()))
    print(taken)
    assert taken["one_step_k0.1"] == taken["one_step_k0.05"] == 1 and taken["two_steps_k2"] == 2 and taken["fifty_steps"] == 50
    assert min(taken["many_steps_a"], taken["many_steps_b"], taken["many_steps_c"]) >= 8


def _aggd_from_data(v):
    """NIQE's estimate from the values themselves (the published estimate_aggd_param)."""
    gam, r_gam = EI.gam_table()
    ls, rs = math.sqrt(np.mean(v[v < 0] ** 2)), math.sqrt(np.mean(v[v > 0] ** 2))
    g = ls / rs
    rhat = np.mean(np.abs(v)) ** 2 / np.mean(v ** 2)
    rn = rhat * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
    alpha = gam[np.argmin((r_gam - rn) ** 2)]
    sc = math.sqrt(math.gamma(1 / alpha) / math.gamma(3 / alpha))
    return alpha, ls * sc, rs * sc


def test_aggd_fit_from_six_numbers_equals_the_fit_from_the_data():
    rng = np.random.default_rng(8)
    for count, skew in ((7056, 1.0), (1764, 1.7), (7056, 0.4)):
        v = rng.standard_normal(count)
        v = np.where(v > 0, v * skew, v) ** 3
        a, bl, br, mean = EI.aggd_from_six(EI._six(v[None, :]), count)
        ra, rbl, rbr = _aggd_from_data(v)
        assert a[0] == ra and abs(bl[0] - rbl) <= 1e-12 * rbl and abs(br[0] - rbr) <= 1e-12 * rbr
        assert abs(mean[0] - (rbr - rbl) * math.gamma(2 / ra) / math.gamma(1 / ra)) <= 1e-12 * abs(mean[0])
    six = EI._six(v[None, :])[0]
    assert six[0] == (v < 0).sum() and six[1] == (v > 0).sum() and abs(six[5] - math.fsum((v * v).tolist())) <= 1e-13 * six[5]
    assert abs(EI.wg_sum(v[None, :])[0] - math.fsum(v.tolist())) <= 1e-12 * np.abs(v).sum() and abs(EI.wg_sum(v, 1024) - math.fsum(v.tolist())) <= 1e-12 * np.abs(v).sum()


def test_det_log_is_log_within_an_ulp():
    x = np.concatenate([np.random.default_rng(0).uniform(1e-5, 255.00001, 100000), [1e-5, 1.0, 255.00001, 1.41, 1.39, 0.70710678, 0.7072, 2.0, 0.5]])
    d = EI.det_log(x)
    assert d[100001] == 0.0 and np.all(np.abs(d - np.log(x)) <= np.maximum(np.spacing(np.abs(np.log(x))), 2.0 ** -60))


@pytest.mark.parametrize("name", list(IC.SIZES))
def test_features_are_finite_and_the_score_is_the_direct_evaluation(name):
    """Every one of the model's 36 x 468 features is finite on every case, so the comparisons of the GPU test leave nothing out; the score equals
    a block-by-block evaluation, does not depend on the order of the blocks, and the package's host part gives the model's numbers."""
    from instarevive_amd import ilniqe
    stats, feat, score = IC.model(name)
    assert stats.shape == (2, 36, 558) and feat.shape == (36, 468) and np.isfinite(stats).all() and np.isfinite(feat).all()
    mu, cov, mean_s, pv = IC.params()
    c = np.stack([pv.T @ (np.minimum(f, 10000.0) - mean_s) for f in feat])
    inv = np.linalg.pinv((cov + np.cov(c, rowvar=False, ddof=1)) / 2.0)
    direct = float(np.mean([math.sqrt((row - mu) @ inv @ (row - mu)) for row in c]))
    assert abs(score - direct) <= 1e-10 * direct
    assert abs(EI.score_features(feat[::-1], IC.params()) - score) <= 1e-10 * score
    assert np.array_equal(ilniqe.features_from_stats(stats), feat) and ilniqe.score(feat, IC.params()) == score


def test_nan_rows_and_the_flat_quarter():
    from instarevive_amd import ilniqe
    stats, feat, score = IC.model(IC.FLAT)
    nan_rows = np.isnan(feat).any(axis=1)
    assert 0 < nan_rows.sum() < 35 and np.isfinite(score)                       # the flat blocks have no AGGD fit of plane 0; the others carry the score
    assert np.array_equal(np.isnan(ilniqe.features_from_stats(stats)), np.isnan(feat))
    assert abs(ilniqe.score(feat, IC.params()) - score) <= 1e-12 * score
    bad = np.full((36, 468), np.nan)
    bad[0] = feat[~nan_rows][0]
    with pytest.raises(ValueError):
        EI.score_features(bad, IC.params())
    with pytest.raises(ilniqe.IlniqeError, match="two complete feature rows"):
        ilniqe.score(bad, IC.params())
    assert np.isnan(ilniqe.score_or_nan(np.zeros((2, 36, 558)), IC.params()))
    big = np.array(IC.model("up_24x24")[1])
    big[3, 7] = 5e4                                                              # infConst
    capped = big.copy()
    capped[3, 7] = 10000.0
    assert EI.score_features(big, IC.params()) == EI.score_features(capped, IC.params())


# ---------------------------------------------------------------------------------------------------------------- the noise floor
def test_noise_floor():
    """The model against itself with the dense DFT product in place of scipy.fft, per statistic kind: what tests/support/ilniqe_cases.py records
    and docs/parity.md shows. The recorded floors are the measured ones (never below, and at most twice them)."""
    floors = {k: 0.0 for k in IC.FLOORS}
    one = more = total = 0
    for name in IC.SIZES:
        a, b = IC.model(name, "scipy"), IC.model(name, "dense")
        for k in IC.KINDS:
            floors[k] = max(floors[k], IC.kind_deviation(b[0], a[0], k))
        floors["score"] = max(floors["score"], abs(b[2] - a[2]) / a[2])
        assert IC.counts_equal(b[0], a[0]), name
        o, m, t = IC.alpha_cells(b[0], a[0])
        one, more, total = one + o, more + m, total + t
    print("floors", {k: f"{v:.3e}" for k, v in floors.items()}, "alpha cells one step", one, "more", more, "of", total)
    assert more == 0 and one / total == IC.ALPHA_SHARE
    for k, v in floors.items():
        assert 0.5 * IC.FLOORS[k] <= v <= IC.FLOORS[k], (k, v, IC.FLOORS[k])


# ---------------------------------------------------------------------------------------------------------------- host code
def test_load_params_reads_mat_and_npz_and_refuses_the_rest(tmp_path):
    from instarevive_amd import ilniqe
    par = IC.params()
    for path in (IC.write_npz(tmp_path / "t.npz"), IC.write_mat(tmp_path / "ILNIQE_templateModel.mat")):
        for load in (ilniqe.load_params, EI.load_params):
            got = load(path)
            assert all(np.array_equal(a, b) for a, b in zip(got, par)) and got[0].shape == (40,) and got[3].shape == (468, 40)
    mu, cov, mean_s, pv = par
    np.savez(tmp_path / "d7.npz", mu_prisparam=mu[:7], cov_prisparam=cov[:7, :7], meanOfSampleData=mean_s, principleVectors=pv[:, :7])
    assert ilniqe.load_params(str(tmp_path / "d7.npz"))[1].shape == (7, 7)      # d comes from the file

    def refused(name, match, **arrays):
        np.savez(tmp_path / name, **arrays)
        with pytest.raises(ilniqe.IlniqeError, match=match):
            ilniqe.load_params(str(tmp_path / name))

    full = dict(mu_prisparam=mu, cov_prisparam=cov, meanOfSampleData=mean_s, principleVectors=pv)
    refused("nokey.npz", r"nokey\.npz.*principleVectors missing", **{k: v for k, v in full.items() if k != "principleVectors"})
    refused("cov.npz", r"cov\.npz.*d x d", **{**full, "cov_prisparam": cov[:, :39]})
    refused("mean.npz", r"mean\.npz.*468 values", **{**full, "meanOfSampleData": mean_s[:467]})
    refused("pv.npz", r"pv\.npz.*468 x d", **{**full, "principleVectors": pv.T})
    refused("nan.npz", r"nan\.npz.*NaN or infinity", **{**full, "mu_prisparam": np.where(np.arange(40) == 3, np.nan, mu)})
    refused("inf.npz", r"inf\.npz.*NaN or infinity", **{**full, "principleVectors": np.where(pv == pv[0, 0], np.inf, pv)})
    from scipy.io import savemat
    savemat(str(tmp_path / "other.mat"), {"mu_prisparam": mu})
    with pytest.raises(ilniqe.IlniqeError, match=r"other\.mat.*templateModel"):
        ilniqe.load_params(str(tmp_path / "other.mat"))
    (tmp_path / "text.mat").write_text("not a mat file")
    with pytest.raises(ilniqe.IlniqeError, match=r"text\.mat.*cannot be read"):
        ilniqe.load_params(str(tmp_path / "text.mat"))
    with pytest.raises(ilniqe.IlniqeError, match=r"void\.npz.*cannot be read"):
        ilniqe.load_params(str(tmp_path / "void.npz"))
    bad = IC.write_mat(tmp_path / "nanmat.mat", (mu, np.where(np.eye(40) > 0, np.nan, cov), mean_s, pv))
    with pytest.raises(ilniqe.IlniqeError, match=r"nanmat\.mat.*NaN or infinity"):
        ilniqe.load_params(bad)


def test_command_lines_parse_and_refuse(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    assert inf.parse_args().ilniqe_params is None and eval_batch.parse_args().ilniqe_params is None and inf.load_ilniqe_params(inf.parse_args()) is None
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))

    def refused(extra, match, mains=(inf.main, eval_batch.main)):
        monkeypatch.setattr(sys, "argv", base + extra)
        for main in mains:
            with pytest.raises(SystemExit, match=match):
                main()

    refused(["--ilniqe_params", str(tmp_path / "nowhere.mat")], "--ilniqe_params .*nowhere.mat: no such file")
    np.savez(tmp_path / "bad.npz", mu_prisparam=np.zeros(3))
    refused(["--ilniqe_params", str(tmp_path / "bad.npz")], r"bad\.npz.*missing")
    refused(["--ilniqe_params", str(tmp_path / "bad.npz"), "--gt", "g", "--niqe_params", str(tmp_path / "nowhere.npz")], r"nowhere\.npz")
    good = IC.write_npz(tmp_path / "good.npz")
    refused(["--ilniqe_params", good, "--shard_tiles"], "--ilniqe_params is not offered together with --shard_tiles", mains=(inf.main,))
    assert touched == []
    monkeypatch.setattr(sys, "argv", base + ["--ilniqe_params", good, "--gt", "g", "--degrade", "r.json"])
    assert all(np.array_equal(a, b) for a, b in zip(inf.load_ilniqe_params(inf.parse_args()), IC.params()))
    monkeypatch.setattr(sys, "argv", ["evaluate_ilniqe.py", "-i", "a", "--ilniqe_params", "p.npz", "--backend", "gpu", "--ntest", "3"])
    seen = {}
    monkeypatch.setattr(EI, "evaluate", lambda *a, **k: seen.update(k, args=a))
    EI.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "p.npz", 3)


def test_report_column_is_there_with_the_flag_and_absent_without(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    old = Report(str(tmp_path / "old.csv"), lpips=True, niqe=True, clipiqa=True)
    old.add("a.png", 30.0, 0.9, 0.1, niqe=4.0, clipiqa=0.5)
    assert old.header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa" and old.write() == ["psnr: 30.00000", "ssim: 0.90000", "lpips: 0.10000", "niqe: 4.00000", "clipiqa: 0.50000"]
    assert (tmp_path / "old.csv").read_text() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa\na.png,30.0,0.9,0.1,4.0,0.5\n"
    new = Report(str(tmp_path / "new.csv"), niqe=True, ilniqe=True, clipiqa=True)
    new.add_scores("b.png", (31.0, 0.8, 5.0, 22.5, 0.25))
    new.add("a.png", 30.0, 0.9, niqe=4.0, clipiqa=0.5, ilniqe=20.0)
    assert new.header() == "file,psnr_y,ssim_y,niqe,ilniqe,clipiqa" and new.write()[3] == "ilniqe: 21.25000"
    assert read_report(str(tmp_path / "new.csv")) == {"a.png": (30.0, 0.9, 4.0, 20.0, 0.5), "b.png": (31.0, 0.8, 5.0, 22.5, 0.25)}
    alone = Report(str(tmp_path / "alone.csv"), ilniqe=True, paired=False)
    alone.add_scores("c.png", (19.0,))
    assert alone.header() == "file,ilniqe" and alone.write() == ["ilniqe: 19.00000"] and read_report(str(tmp_path / "alone.csv")) == {"c.png": (19.0,)}
    assert alone.unscored((float("nan"),)) == "ilniqe" and new.unscored((1.0, 1.0, float("nan"), float("nan"), 1.0)) == "niqe"
    with pytest.raises(MetricsError, match="IL-NIQE value"):
        old.add("x.png", 1.0, 1.0, 0.1, niqe=1.0, clipiqa=1.0, ilniqe=1.0)
    with pytest.raises(MetricsError, match="IL-NIQE value"):
        alone.add("x.png")
    with pytest.raises(MetricsError):
        Report(None, paired=False)


def test_header_symbols_and_build_list_move_together():
    L, lib = _library()
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    names = ["ir_ilniqe_plan_bytes", "ir_ilniqe_plan", "ir_ilniqe_configure", "ir_ilniqe_stats", "ir_op_dft2_f64", "ir_op_weibull_fit"]
    for name in names:
        assert f"int {name}(" in header and name in L.SYMBOLS and hasattr(lib, name), name
    assert "IR_STAGE_ILNIQE = 27" in header and L.STAGE_ILNIQE == 27 and "IR_STAGE_ILNIQE_DFT = 26" in header and L.STAGE_ILNIQE_DFT == 26
    assert lib.ir_abi_version() == 3   # the entry points are additive
    from instarevive_amd import build
    assert "ilniqe.hip" in build.SOURCES
    flags = build.FLAGS + build.FILE_FLAGS.get("ilniqe.hip", [])
    assert [f for f in flags if f.startswith("-ffp-contract")][-1] == "-ffp-contract=off"   # plane 0 has to equal the model's bits


def test_workspace_needs_no_context_and_calls_refuse_without_one():
    L, lib = _library()
    from instarevive_amd import ilniqe
    ws = lambda n, h, w: lib.ir_workspace_bytes(None, L.STAGE_ILNIQE, n, h, w, 0, 0, 0)
    planes = (109 + 2 + 6 + 1.5) * 504 * 504 * 8
    assert planes + 504 * 3 * 700 * 8 <= ws(1, 40, 700) <= planes + 504 * 3 * 700 * 8 + 512 and ws(5, 40, 700) == ws(1, 40, 700) == ilniqe.ws_bytes(1, 40, 700)
    assert ws(0, 40, 700) == 0 and ws(1, 1, 700) == 0 and ws(1, 40, 1) == 0
    dws = lambda s: lib.ir_workspace_bytes(None, L.STAGE_ILNIQE_DFT, 1, s, s, 0, 0, 0)
    assert dws(504) == 2 * 504 * 504 * 8 and dws(252) == 2 * 252 * 252 * 8 and dws(256) == 0 and ilniqe.dft_ws_bytes(504) == dws(504)
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is launched
    assert lib.ir_ilniqe_stats(None, None, fake, 24, 72, 1, 24, 24, fake, fake, fake, 1 << 30) == -1
    assert lib.ir_op_dft2_f64(None, None, fake, None, 504, 0, fake, fake, fake, 1 << 30) == -1
    assert lib.ir_op_weibull_fit(None, None, fake, 1, 100, fake) == -1 and lib.ir_ilniqe_configure(None) == -1
