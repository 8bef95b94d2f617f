"""FID without a GPU: the two resizes bit for bit against Pillow and torch, the fp32 host model against the float64 model (from which the gates
of tests/test_fid_gpu.py are measured), every known way to get FID wrong against the feature gate, the Frechet distance against closed forms
and against pytorch-fid's own arithmetic, the loader, the feature files, the resize tables of the library and the ABI.

Figures of this file (recorded in docs/parity.md): the fp32 host model is 2.0e-7 .. 2.7e-7 off the float64 model over the nine cases
(max_c |f - ref| / max_c |ref|), so the feature gate is 2.2e-6; the block gates are 4.4e-7 .. 2.6e-6."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import fid_model as FM

EF = FM.EF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(299, 299), (300, 301), (64, 48), (512, 384), (37, 1000)]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _pillow(plane):
    return np.asarray(Image.fromarray(np.ascontiguousarray(plane, np.float32), "F").resize((EF.SIZE, EF.SIZE), Image.BICUBIC))


@pytest.mark.parametrize("h,w", SIZES)
def test_clean_resize_has_pillows_bits(h, w):
    img = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = EF.resize_clean(img)
    want = np.clip(np.stack([_pillow(img[:, :, c]) for c in range(3)], -1), 0, 255)
    assert got.shape == (299, 299, 3) and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))
    if (h, w) == (299, 299):
        assert np.array_equal(got, img.astype(np.float32))


def test_clean_resize_has_pillows_bits_at_2048():
    """One plane; the support is 28 taps."""
    plane = np.random.default_rng(2048).integers(0, 256, (2048, 2048), dtype=np.uint8)
    assert EF.clean_tables(2048)[1].shape[1] == 29 and EF.clean_tables(2048)[0][:, 1].max() == 28
    got = EF.resize_clean(np.repeat(plane[:, :, None], 3, 2))
    want = np.clip(_pillow(plane), 0, 255)
    for c in range(3):
        assert np.array_equal(_bits(got[:, :, c]), _bits(want))


@pytest.mark.parametrize("h,w", SIZES + [(2048, 2048)])
def test_legacy_resize_has_torchs_bits(h, w):
    img = np.random.default_rng(h * 5 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    x = torch.from_numpy(img).permute(2, 0, 1)[None].float() / 255
    want = torch.nn.functional.interpolate(x, (EF.SIZE, EF.SIZE), mode="bilinear", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert np.array_equal(_bits(EF.resize_legacy(img)), _bits(want))


@pytest.mark.parametrize("mode", ["clean", "legacy"])
@pytest.mark.parametrize("h,w", [(300, 301), (64, 48), (37, 1000), (2048, 2048)])
def test_library_tables_are_the_models(h, w, mode):
    """ir_fid_resize_plan (host code of the library, no GPU) gives the numpy model's bounds and coefficients to the bit."""
    from instarevive_amd import fid as G
    xb, xk, yb, yk = G.plan_tables(G.resize_plan(h, w, mode), h, w, mode)
    tab = EF.clean_tables if mode == "clean" else EF.legacy_tables
    for (b, k), size in (((xb, xk), w), ((yb, yk), h)):
        wb, wk = tab(size)
        assert np.array_equal(b, wb)
        assert np.array_equal(k.view(np.uint64), np.ascontiguousarray(wk, np.float64).view(np.uint64))
    lib = L.load_library()
    assert lib.ir_fid_resize_plan_bytes(0, 5, 0) == 0 and lib.ir_fid_resize_plan_bytes(5, 5, 2) == 0
    assert lib.ir_fid_resize_plan(h, w, 0, None, 1 << 20) == -1
    buf = np.zeros(8, np.int64)
    assert lib.ir_fid_resize_plan(h, w, 0, C.c_void_p(buf.ctypes.data), 64) == -1 and not buf.any()


def test_host_model_against_the_float64_model():
    dev, blocks = FM.host_deviation()
    for n in FM.NAMES:
        print(f"{n}: fp32 host model off by {FM.measure(FM.host(n)[0], FM.reference(n)[0]):.3e}")
    print(f"feature gate {FM.feature_gate():.3e}; block gates", " ".join(f"{g:.2e}" for g in FM.block_gates()))
    assert 0 < dev < 1e-5 and np.all(blocks > 0) and np.all(blocks < 1e-5)   # fp32 rounding, not a different model
    f, means = FM.reference("64x48")
    assert f.shape == (2048,) and means.shape == (FM.OFFSETS[-1],) == (L.FID_BLOCK_CHANNELS,)
    assert np.array_equal(f, means[FM.OFFSETS[-2]:])
    assert (f > 0).mean() > 0.5   # the seeded network is alive at its end
    assert EF.macs_per_image() == 5711168096


def _variant_features(name, mode_input=None, **variant):
    x = mode_input if mode_input is not None else EF.network_input(FM.image(name), "clean")
    return EF.InceptionFID(FM.weights(), "fp32", **variant).features(x[None])[0][0]


@pytest.mark.parametrize("what", ["count_include_pad", "average_in_7c", "eps_1e-5", "swapped_branches", "v_over_255", "no_antialias"])
def test_every_known_mistake_lands_outside_the_gate(what):
    name = "512x384"
    img = FM.image(name)
    if what == "count_include_pad":
        f = _variant_features(name, count_include_pad=True)
    elif what == "average_in_7c":
        f = _variant_features(name, last_pool_max=False)
    elif what == "eps_1e-5":
        f = _variant_features(name, eps=1e-5)
    elif what == "swapped_branches":
        f = _variant_features(name, swap_branches=True)
    elif what == "v_over_255":
        f = _variant_features(name, np.float32(2) * EF.resize_clean(img) / np.float32(255) - np.float32(1))
    else:
        r = img.astype(np.float32)   # Pillow's own kernel (a = -0.5) and passes, only without the widening of the support
        r = EF._clean_pass(r.transpose(1, 0, 2), *EF.clean_tables(img.shape[1], antialias=False)).transpose(1, 0, 2)
        r = EF._clean_pass(r, *EF.clean_tables(img.shape[0], antialias=False))
        f = _variant_features(name, (np.clip(r, 0, 255) - np.float32(128)) / np.float32(128))
    off = FM.measure(f, FM.reference(name)[0])
    print(f"{what}: {off:.3e} against the gate {FM.feature_gate():.3e}")
    assert off > FM.feature_gate()


# ---------------------------------------------------------------- the Frechet distance
def _sqrtm_fid(mu1, s1, mu2, s2):
    """pytorch-fid's arithmetic."""
    from scipy import linalg
    covmean = linalg.sqrtm(s1.dot(s2))
    if isinstance(covmean, tuple):
        covmean = covmean[0]
    if not np.isfinite(covmean).all():
        off = np.eye(s1.shape[0]) * 1e-6
        covmean = linalg.sqrtm((s1 + off).dot(s2 + off))
    covmean = np.real(covmean)
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def _closed_forms(D, seed):
    """[(name, mu1, s1, mu2, s2, exact)]"""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D)
    mu, delta = rng.normal(0, 1, D), rng.normal(0, 0.3, D)
    q, _ = np.linalg.qr(rng.normal(0, 1, (D, D)))
    x = rng.normal(0, 1, (4 * D, D)) * np.sqrt(a)
    s = np.cov(x, rowvar=False)
    diag = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    return [("identical", mu, s, mu, s, 0.0), ("mean shift", mu, s, mu + delta, s, float(delta @ delta)),
            ("diagonal", mu, np.diag(a), mu, np.diag(b), diag), ("rotated", q @ mu, q @ np.diag(a) @ q.T, q @ mu, q @ np.diag(b) @ q.T, diag)]


def _relative(v, exact, s1, s2):
    return abs(v - exact) / (np.trace(s1) + np.trace(s2))


def test_frechet_distance_closed_forms():
    """Tolerance: 8 x the largest deviation pytorch-fid's sqrtm form shows on the D = 64 cases, relative to tr s1 + tr s2 (recorded in
    docs/parity.md); the D = 2048 case (diagonal, rotated) takes the same relative tolerance - sqrtm at that size takes minutes."""
    pytest.importorskip("scipy")
    cases = _closed_forms(64, 11)
    theirs = max(_relative(_sqrtm_fid(m1, s1, m2, s2), ex, s1, s2) for _, m1, s1, m2, s2, ex in cases)
    tol = 8.0 * theirs
    print(f"sqrtm form off by {theirs:.3e} of tr s1 + tr s2 at most; tolerance {tol:.3e}")
    assert 0 < tol < 1e-6
    for name, m1, s1, m2, s2, ex in cases + _closed_forms(2048, 12)[3:]:
        got = EF.frechet_distance(m1, s1, m2, s2)
        print(f"D = {m1.size} {name}: {got:.12g} against {ex:.12g}, off by {_relative(got, ex, s1, s2):.3e}")
        assert np.isfinite(got) and _relative(got, ex, s1, s2) <= tol, name


def test_frechet_distance_agrees_with_the_sqrtm_form_at_full_rank():
    pytest.importorskip("scipy")
    rng = np.random.default_rng(5)
    D = 64
    mix = rng.normal(0, 1, (D, D)) / np.sqrt(D)
    a, b = rng.normal(0, 1, (4 * D, D)) @ mix, rng.normal(0.1, 1.2, (4 * D, D))
    (m1, s1), (m2, s2) = EF.statistics(a), EF.statistics(b)
    got, want = EF.frechet_distance(m1, s1, m2, s2), _sqrtm_fid(m1, s1, m2, s2)
    print(f"eigh form {got:.12g}, sqrtm form {want:.12g}")
    assert abs(got - want) <= 1e-9 * (np.trace(s1) + np.trace(s2))   # both are fp64 evaluations of one well-conditioned quantity
    assert got == EF.fid_of(a, b) and abs(EF.frechet_distance(m2, s2, m1, s1) - got) <= 1e-9 * (np.trace(s1) + np.trace(s2))


def test_singular_covariances_give_a_real_finite_value():
    rng = np.random.default_rng(6)
    a, b = rng.normal(0, 1, (6, 2048)), rng.normal(0.2, 1, (7, 2048))
    v = EF.fid_of(a, b)
    assert isinstance(v, float) and np.isfinite(v) and v >= 0
    assert abs(EF.fid_of(a, a)) <= 1e-9 * 2 * np.trace(np.cov(a, rowvar=False))
    assert "rank-deficient" in EF.rank_deficient_note(6) and "equal N" in EF.rank_deficient_note(6) and EF.rank_deficient_note(2048) is None


def test_fewer_than_two_files_is_an_error_that_says_so():
    with pytest.raises(EF.FidError, match="at least 2 files"):
        EF.statistics(np.zeros((1, 2048)))
    with pytest.raises(EF.FidError, match="at least 2 files"):
        EF.fid_of(np.zeros((5, 8)), np.zeros((0, 8)))


def test_feature_files_merge_to_the_unsplit_set(tmp_path):
    from instarevive_amd import fid as G
    rng = np.random.default_rng(7)
    feats = rng.normal(0, 1, (9, 2048))
    names = [f"img_{i:02d}.png" for i in range(9)]
    whole, parts = G.FeatureSet(), [G.FeatureSet(), G.FeatureSet()]
    for i in rng.permutation(9):
        whole.add(names[i], feats[i])
        parts[i % 2].add(names[i], feats[i])
    for k, p in enumerate(parts):
        p.save(tmp_path / f"fid_features.rank{k}.npz")
    merged = G.merge([G.FeatureSet.load(tmp_path / f"fid_features.rank{k}.npz") for k in range(2)])
    one = G.merge([whole])
    assert merged.names == one.names == names and np.array_equal(merged.features, one.features) and np.array_equal(merged.features, feats)
    ref = rng.normal(0, 1, (5, 2048))
    assert G.frechet_distance(*G.statistics(merged.features), *G.statistics(ref)) == G.frechet_distance(*G.statistics(feats), *G.statistics(ref))
    mu, sigma = G.statistics(ref)
    np.savez(tmp_path / "stats.npz", mu=mu, sigma=sigma)
    lm, ls = G.load_stats(tmp_path / "stats.npz")
    assert np.array_equal(lm, mu) and np.array_equal(ls, sigma)
    np.savez(tmp_path / "bad.npz", mu=mu)
    with pytest.raises(G.FidError, match="mu and sigma"):
        G.load_stats(tmp_path / "bad.npz")
    with pytest.raises(G.FidError, match="2048"):
        whole.add("short", np.zeros(7))


def test_loader_forms_agree_and_name_what_is_wrong(tmp_path):
    from instarevive_amd import fid as G
    w, sd = FM.weights(), FM.state_dict()
    torch.save(sd, tmp_path / "pt_inception.pth")
    np.savez(tmp_path / "fid.npz", **{k: v.numpy() for k, v in w.items()})
    assert G.tensor_names() == list(w) and len(w) == 5 * 94
    for got in (G.load_weights(sd), G.load_weights(str(tmp_path / "pt_inception.pth")), G.load_weights(str(tmp_path / "fid.npz")), G.load_weights(dict(w))):
        assert list(got) == list(w) and all(torch.equal(got[k], w[k]) and got[k].dtype == torch.float32 for k in w)
    broken = dict(sd)
    del broken["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(KeyError, match="Mixed_6c.branch7x7dbl_3.bn.running_var"):
        G.load_weights(broken)
    broken = dict(sd)
    broken["Mixed_7a.branch7x7x3_2.conv.weight"] = torch.zeros((192, 192, 7, 1))
    with pytest.raises(ValueError, match=r"Mixed_7a.branch7x7x3_2.conv.weight.*\(192, 192, 1, 7\)"):
        G.load_weights(broken)
    own = dict(w)
    del own["fid.Conv2d_3b_1x1.bn_b"]
    with pytest.raises(KeyError, match="fid.Conv2d_3b_1x1.bn_b"):
        EF.InceptionFID(own)


def test_tool_scores_feature_files(tmp_path, capsys):
    rng = np.random.default_rng(8)
    a, b = EF.FeatureSet(), EF.FeatureSet()
    for i in range(5):
        a.add(f"{i}.png", rng.normal(0, 1, 2048))
        b.add(f"{i}.png", rng.normal(0.1, 1, 2048))
    a.save(tmp_path / "a.npz", gt_names=np.array(b.names), gt_features=b.features)
    assert EF.main(["--features", str(tmp_path / "a.npz")]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert "rank-deficient" in out[0] and out[-1] == f"fid: {EF.fid_of(a.features, b.features):.5f}"
    mu, sigma = EF.statistics(b.features)
    np.savez(tmp_path / "s.npz", mu=mu, sigma=sigma)
    assert EF.main(["--features", str(tmp_path / "a.npz"), "--stats", str(tmp_path / "s.npz")]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == out[-1]
    one = EF.FeatureSet()
    one.add("x", np.zeros(2048))
    one.save(tmp_path / "one.npz")
    assert EF.main(["--features", str(tmp_path / "one.npz"), "--stats", str(tmp_path / "s.npz")]) == 2
    assert "at least 2 files" in capsys.readouterr().err


def test_command_lines_refuse_the_flag_without_a_reference_before_anything_loads(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    for a in (inf.parse_args(), eval_batch.parse_args()):
        assert a.fid_model is None and a.fid_stats is None and a.fid_features_out is None and a.fid_resize == "clean"
    assert inf.load_fid(inf.parse_args()) == (None, None)
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    np.savez(tmp_path / "w.npz", **{k: v.numpy() for k, v in FM.weights().items()})
    good = str(tmp_path / "w.npz")
    mu, sigma = EF.statistics(np.random.default_rng(1).normal(0, 1, (4, 2048)))
    np.savez(tmp_path / "s.npz", mu=mu, sigma=sigma)
    np.savez(tmp_path / "nostats.npz", mu=mu)

    def refused(extra, match):
        monkeypatch.setattr(sys, "argv", base + extra)
        for main in (inf.main, eval_batch.main):
            with pytest.raises(SystemExit, match=match) as e:
                main()
            assert "\n" not in str(e.value)

    refused(["--fid_model", good], "--fid_model needs a reference set: give --gt .or --degrade., or --fid_stats")
    refused(["--fid_stats", str(tmp_path / "s.npz")], "--fid_stats needs --fid_model")
    refused(["--fid_features_out", "f.npz"], "--fid_features_out needs --fid_model")
    refused(["--fid_resize", "legacy"], "--fid_resize needs --fid_model")
    refused(["--fid_model", str(tmp_path / "nowhere.pth"), "--gt", "g"], "nowhere.pth: no such file")
    refused(["--fid_model", good, "--fid_stats", str(tmp_path / "nowhere.npz")], "nowhere.npz: no such file")
    refused(["--fid_model", good, "--fid_stats", str(tmp_path / "nostats.npz")], "nostats.npz.*mu and sigma")
    np.savez(tmp_path / "part.npz", **{k: v.numpy() for k, v in FM.weights().items() if k != "fid.Mixed_7c.branch_pool.bn_var"})
    refused(["--fid_model", str(tmp_path / "part.npz"), "--gt", "g"], r"part\.npz.*fid\.Mixed_7c\.branch_pool\.bn_var missing")
    monkeypatch.setattr(sys, "argv", base + ["--fid_model", good, "--gt", "g", "--shard_tiles"])
    with pytest.raises(SystemExit, match="--fid_model is not offered together with --shard_tiles"):
        inf.main()
    assert touched == []
    for extra in (["--degrade"], ["--fid_stats", str(tmp_path / "s.npz")]):   # --degrade: the input folder is the ground truth; --fid_stats needs no --gt
        monkeypatch.setattr(sys, "argv", base + ["--fid_model", good] + extra)
        w, st = inf.load_fid(inf.parse_args())
        assert list(w) == EF.tensor_names() and (st is None) == (extra[0] == "--degrade")


def test_run_writes_rank_files_and_rank_0_merges_them(tmp_path):
    """fid.Run over two ranks in one process (no group: the barrier is skipped): each writes fid_features.rank<k>.npz, rank 0 makes the value
    of the merged set - the value of the unsplit set."""
    from instarevive_amd import fid as G
    rng = np.random.default_rng(9)
    pred, gt = rng.normal(0, 1, (7, 2048)), rng.normal(0.1, 1, (7, 2048))
    names = [f"f{i}.png" for i in range(7)]
    path = G.Run.default_path(str(tmp_path))
    assert path == str(tmp_path / "fid_features.npz")
    runs = [G.Run(path, None, k, 2) for k in range(2)]
    for k, r in enumerate(runs):
        idx = list(range(k, 7, 2))
        r.add([names[i] for i in idx], {"fid": pred[idx], "fid_gt": gt[idx]})
    runs[1].add(["left.png"], None)
    log = []
    assert runs[1].finish(log.append) is None and runs[1].left_out == 1
    value = runs[0].finish(log.append)
    assert value == EF.fid_of(pred, gt) and log[-1] == f"fid: {value:.5f}" and (tmp_path / "fid.txt").read_text() == log[-1] + "\n"
    assert sorted(os.listdir(tmp_path)) == ["fid.txt", "fid_features.rank0.npz", "fid_features.rank1.npz"]
    assert any("4 files entered the set, 0 did not" in ln for ln in log) and any("3 files entered the set, 1 did not" in ln for ln in log)
    one = G.Run(str(tmp_path / "x" / "one.npz"), EF.statistics(gt))
    one.add(names[:1], {"fid": pred[:1], "fid_gt": None})
    assert one.finish(log.append) is None and "at least 2 files" in log[-1]


def test_abi_exports_the_fid_symbols():
    lib = L.load_library()
    for s in ("ir_fid_resize_plan_bytes", "ir_fid_resize_plan", "ir_fid_configure", "ir_fid_features"):
        assert s in L.SYMBOLS and hasattr(lib, s)
    assert lib.ir_abi_version() == 3
    need = int(lib.ir_workspace_bytes(None, L.STAGE_FID, 1, 0, 0, 0, 0, 0))
    assert need % 256 == 0 and need >= 4 * (299 * 299 * 4 + 4 * 147 * 147 * 64)
    assert int(lib.ir_workspace_bytes(None, L.STAGE_FID, 3, 512, 384, 0, 0, 0)) == int(lib.ir_workspace_bytes(None, L.STAGE_FID, 3, 0, 0, 0, 0, 0)) > 2 * need
    assert int(lib.ir_workspace_bytes(None, L.STAGE_FID, 0, 0, 0, 0, 0, 0)) == 0
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    assert "IR_STAGE_FID = 24" in header and "int ir_fid_features(" in header
