"""DISTS without a GPU: the host model tools/evaluate_pairs.py::DISTS against its float64 form on every case, what the gates of
tests/support/dists_model.py can tell apart (the planted bugs), the weight-file forms, the library's host-only table, the report and the
command-line refusals."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.support import dists_model as DM
from tests.support.metrics_model import EP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp32_host_model_against_the_float64_model_on_every_case():
    """The yardstick of the gates: the fp32 model is a few 1e-8 .. 1e-7 off in the score (mostly its last subtraction next to 1); the flat case
    is ill-conditioned (its variances are rounding noise against c2 = 1e-6) and orders of magnitude worse, which is why it stays out of the pool."""
    for name in DM.NAMES:
        print(f"{name}: float64 {DM.reference(name)[0]:.17g}, fp32 off by {DM.host_deviation(name):.3e}")
    pooled = max(DM.host_deviation(n) for n in DM.pooled_names())
    assert 0 < pooled < 1e-6 and DM.score_gate(DM.NAMES[0]) == DM.GATE_FACTOR * pooled
    assert DM.host_deviation(DM.FLAT) > 100 * pooled and DM.score_gate(DM.FLAT) == DM.GATE_FACTOR * DM.host_deviation(DM.FLAT)
    assert all(0 <= DM.reference(n)[0] < 1 for n in DM.NAMES)
    g = DM.moment_gate(DM.NAMES[0])
    assert g.shape == (6, 5) and np.all(g > 0) and np.all(g < 1e-3)


def test_identical_images_give_exactly_zero_in_the_model():
    assert DM.reference("33x18_same")[0] == 0.0
    a = DM.pair("97x130_ramps")[0]
    net = DM.model()
    assert float(net(DM.unit(a), DM.unit(a.copy()))[0]) == 0.0


def test_dead_stage_scores_one_from_the_constants_alone():
    m = DM.reference("64x64_dead5")[1]
    assert np.all(m[DM.OFFSETS[5]:] == 0.0) and np.any(DM.evaluate("64x64_dead5")[1][DM.OFFSETS[4]:DM.OFFSETS[5]] != 0.0)
    assert np.isfinite(DM.reference("64x64_dead5")[0])


def test_the_model_is_the_published_construction():
    """An independent torch.nn construction of the definition: nn.Conv2d stages with the L2 pooling layer written as the published module writes
    it (hanning(5)[1:-1], depthwise conv2d of x ** 2, stride 2, padding 1), alpha and beta split per map and divided by their sum."""
    w = DM.weights()
    a, b = DM.pair("17x33_near")
    filt = np.hanning(5)[1:-1]
    g = torch.tensor(filt[:, None] * filt[None, :] / (filt[:, None] * filt[None, :]).sum(), dtype=torch.float64)

    def feats(img):
        x = DM.unit(img)
        h = ((x - torch.tensor(EP.DISTS_MEAN).view(1, 3, 1, 1)) / torch.tensor(EP.DISTS_STD).view(1, 3, 1, 1)).double()
        outs, k = [x.double()], 0
        for s, count in enumerate((2, 2, 3, 3, 3)):
            if s:
                c = h.shape[1]
                h = (F.conv2d(h ** 2, g[None, None].repeat(c, 1, 1, 1), stride=2, padding=1, groups=c) + 1e-12).sqrt()
            for _ in range(count):
                k += 1
                h = F.relu(F.conv2d(h, w[f"dists.c{k}.w"].double(), w[f"dists.c{k}.b"].double(), padding=1))
            outs.append(h)
        return outs

    alpha, beta = w["dists.alpha"].double().view(1, -1, 1, 1), w["dists.beta"].double().view(1, -1, 1, 1)
    wsum = alpha.sum() + beta.sum()
    d1 = d2 = 0
    for fx, fy, al, be in zip(feats(a), feats(b), torch.split(alpha / wsum, DM.CHNS, 1), torch.split(beta / wsum, DM.CHNS, 1)):
        mx, my = fx.mean([2, 3], keepdim=True), fy.mean([2, 3], keepdim=True)
        s1 = (2 * mx * my + 1e-6) / (mx ** 2 + my ** 2 + 1e-6)
        d1 = d1 + (al * s1).sum(1, keepdim=True)
        vx, vy = ((fx - mx) ** 2).mean([2, 3], keepdim=True), ((fy - my) ** 2).mean([2, 3], keepdim=True)
        cxy = (fx * fy).mean([2, 3], keepdim=True) - mx * my
        d2 = d2 + (be * (2 * cxy + 1e-6) / (vx + vy + 1e-6)).sum(1, keepdim=True)
    want = float(1 - (d1 + d2).squeeze())
    assert abs(want - DM.reference("17x33_near")[0]) < 1e-14
    sizes = [tuple(f.shape[2:]) for f in feats(a)]
    assert sizes == [(17, 33), (17, 33), (9, 17), (5, 9), (3, 5), (2, 3)] and sum(DM.CHNS) == 1475


def test_every_planted_bug_misses_the_gate():
    """Each way to get DISTS wrong moves at least one small case's score beyond that case's gate; the smallest margin is printed."""
    for bug in DM.PLANTED_BUGS:
        ratio = {n: abs(DM.bugged_score(n, bug) - DM.reference(n)[0]) / DM.score_gate(n) for n in DM.SMALL}
        best = max(ratio, key=ratio.get)
        print(f"{bug}: {ratio[best]:.1f} x the gate on {best}")
        assert ratio[best] > 1.5, (bug, ratio)


def test_library_table_is_the_models_roundings():
    from instarevive_amd import dists
    tab = dists.scaling_table()
    v = torch.arange(256, dtype=torch.float32) / 255.0
    want = ((v.view(1, 1, 256) - torch.tensor(EP.DISTS_MEAN).view(1, 3, 1)) / torch.tensor(EP.DISTS_STD).view(1, 3, 1))[0].numpy()
    assert tab.dtype == np.float32 and np.array_equal(tab, want)


def test_header_symbols_and_build_list_move_together():
    from instarevive_amd import _lib
    from instarevive_amd.build import FILE_FLAGS, SOURCES
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    for s in ("ir_dists_scale_table", "ir_dists_configure", "ir_dists"):
        assert s in _lib.SYMBOLS and f"int {s}(" in header
        assert hasattr(_lib.load_library(), s)
    assert "IR_STAGE_DISTS = 23" in header and _lib.STAGE_DISTS == 23 and _lib.DISTS_NOT_CONFIGURED == -14 and "-14 when" in header
    assert "dists.hip" in SOURCES and FILE_FLAGS["dists.hip"] == ["-ffp-contract=off"]
    lib = _lib.load_library()
    assert lib.ir_workspace_bytes(None, 23, 1, 2048, 2048, 0, 0, 0) // 2 ** 20 in range(4096, 4096 + 16)   # four stage-1 maps: 4.3 GB, and the sums
    assert lib.ir_workspace_bytes(None, 23, 1, 15, 64, 0, 0, 0) == 0


def test_the_weight_file_forms_load_to_the_same_tensors(tmp_path):
    from instarevive_amd import dists
    w = DM.weights()
    ab, none = DM.state_dicts(w, "module")
    torch.save(ab, tmp_path / "module.pth")
    ab2, vgg = DM.state_dicts(w, "vgg")
    torch.save(ab2, tmp_path / "ab.pth")
    torch.save(vgg, tmp_path / "vgg.pth")
    np.savez(tmp_path / "w.npz", **{k: v.numpy() for k, v in w.items()})
    forms = [dists.load_weights(str(tmp_path / "module.pth")), dists.load_weights(str(tmp_path / "ab.pth"), str(tmp_path / "vgg.pth")),
             dists.load_weights(str(tmp_path / "w.npz")), dists.load_weights(ab), dists.load_weights(w)]
    assert none is None and "stage2.4.filter" in ab and "classifier.0.weight" in vgg
    for got in forms:
        assert list(got) == dists.tensor_names() and all(torch.equal(got[k], w[k]) and got[k].dtype == torch.float32 for k in w)
    with pytest.raises(KeyError, match="features.0"):
        dists.load_weights(str(tmp_path / "ab.pth"))
    with pytest.raises(KeyError, match="beta"):
        dists.load_weights({k: v for k, v in ab.items() if k != "beta"})
    bad = dict(ab)
    bad["stage3.12.weight"] = bad["stage3.12.weight"][:, :128]
    with pytest.raises(ValueError, match="features.12"):
        dists.load_weights(bad)
    np.savez(tmp_path / "part.npz", **{k: v.numpy() for k, v in w.items() if k != "dists.c7.b"})
    with pytest.raises(KeyError, match=r"part\.npz: dists\.c7\.b missing"):
        dists.load_weights(str(tmp_path / "part.npz"))


def test_report_carries_dists_last(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    rep = Report(str(tmp_path / "r.csv"), lpips=True, niqe=True, clipiqa=True, musiq=True, maniqa=True, dists=True)
    assert rep.header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq,maniqa,dists"
    rep.add_scores("b.png", (30.0, 0.9, 0.1, 4.0, 0.5, 60.0, 0.25, 0.125))
    rep.add("a.png", psnr=31.0, ssim=0.8, lpips=0.2, niqe=5.0, clipiqa=0.25, musiq=50.0, maniqa=0.75, dists=0.375)
    assert rep.write()[-1] == "dists: 0.25000"
    assert read_report(str(tmp_path / "r.csv"))["a.png"] == (31.0, 0.8, 0.2, 5.0, 0.25, 50.0, 0.75, 0.375)
    plain = Report(str(tmp_path / "p.csv"), dists=True)
    assert plain.header() == "file,psnr_y,ssim_y,dists" and Report(None, lpips=True, dists=True).header() == "file,psnr_y,ssim_y,lpips,dists"
    plain.add_scores("x.png", (30.0, 0.9, 0.5))
    assert plain.write() == ["psnr: 30.00000", "ssim: 0.90000", "dists: 0.50000"] and read_report(str(tmp_path / "p.csv")) == {"x.png": (30.0, 0.9, 0.5)}
    nan = float("nan")
    assert plain.unscored((30.0, 0.9, nan)) == "dists" and plain.unscored((30.0, 0.9, 0.5)) is None
    assert rep.unscored((30.0, 0.9, 0.1, 4.0, 0.5, 60.0, nan, nan)) == "maniqa"   # dists is looked at last
    with pytest.raises(MetricsError):
        Report(None, dists=True, niqe=True, paired=False)
    with pytest.raises(MetricsError):
        Report(None).add("x", psnr=1.0, ssim=1.0, dists=0.5)
    with pytest.raises(MetricsError):
        plain.add("x", psnr=1.0, ssim=1.0)
    assert Report(None).header() == "file,psnr_y,ssim_y" and "file,psnr_y,ssim_y,dists" not in Report.HEADERS + Report.HEADERS_MANIQA


def test_command_lines_refuse_the_flag_alone_before_anything_loads(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    for a in (inf.parse_args(), eval_batch.parse_args()):
        assert a.dists_model is None and a.dists_vgg is None
    assert inf.load_dists_weights(inf.parse_args()) is None
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    np.savez(tmp_path / "w.npz", **{k: v.numpy() for k, v in DM.weights().items()})
    good = str(tmp_path / "w.npz")

    def refused(extra, match):
        monkeypatch.setattr(sys, "argv", base + extra)
        for main in (inf.main, eval_batch.main):
            with pytest.raises(SystemExit, match=match) as e:
                main()
            assert "\n" not in str(e.value)

    refused(["--dists_model", good], "--dists_model scores against ground truth: give --gt")
    refused(["--dists_vgg", good], "--dists_vgg needs --dists_model")
    refused(["--dists_model", str(tmp_path / "nowhere.pth"), "--gt", "g"], "nowhere.pth: no such file")
    refused(["--dists_model", good, "--dists_vgg", str(tmp_path / "novgg.pth"), "--gt", "g"], "novgg.pth: no such file")
    np.savez(tmp_path / "part.npz", **{k: v.numpy() for k, v in DM.weights().items() if k != "dists.alpha"})
    refused(["--dists_model", str(tmp_path / "part.npz"), "--gt", "g"], r"part\.npz.*dists\.alpha missing")
    monkeypatch.setattr(sys, "argv", base + ["--dists_model", good, "--gt", "g", "--shard_tiles"])
    with pytest.raises(SystemExit, match="--dists_model is not offered together with --shard_tiles"):
        inf.main()
    assert touched == []
    monkeypatch.setattr(sys, "argv", base + ["--dists_model", good, "--degrade"])   # --degrade: the input folder is the ground truth
    got = inf.load_dists_weights(inf.parse_args())
    assert list(got) == __import__("instarevive_amd.dists", fromlist=["x"]).tensor_names()


def test_evaluate_pairs_scores_a_folder_with_the_host_model(tmp_path, monkeypatch):
    """tools/evaluate_pairs.py --dists_model: the `dists:` line is the mean of class DISTS over the pairs, behind the other lines."""
    w = DM.weights()
    ab, _ = DM.state_dicts(w, "module")
    torch.save(ab, tmp_path / "dists.pth")
    from PIL import Image
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    pairs = [DM.pair("17x33_near"), DM.pair("35x67_noise")]
    for i, (a, b) in enumerate(pairs):
        Image.fromarray(a).save(tmp_path / "a" / f"{i}.png")
        Image.fromarray(b).save(tmp_path / "b" / f"{i}.png")
    net = EP.DISTS(str(tmp_path / "dists.pth"))
    lines = []
    res = EP.evaluate(str(tmp_path / "a"), str(tmp_path / "b"), log=lines.append, dists=net)
    want = np.mean([float(net(DM.unit(a), DM.unit(b))[0]) for a, b in pairs])
    assert res["dists"] == want and lines[-1] == f"dists: {want:.5f}" and [ln.split(":")[0] for ln in lines[1:]] == ["psnr", "ssim", "dists"]
    assert abs(want - np.mean([DM.reference("17x33_near")[0], DM.reference("35x67_noise")[0]])) < 1e-6
    assert "dists" not in EP.evaluate(str(tmp_path / "a"), str(tmp_path / "b"), log=lines.append)
    monkeypatch.setattr(sys, "argv", ["evaluate_pairs.py", "-i", "a", "-r", "b", "--dists_vgg", "v.pth"])
    with pytest.raises(SystemExit, match="--dists_vgg needs --dists_model"):
        EP.main()
