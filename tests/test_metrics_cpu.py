"""ir_metrics_y and its host side without a GPU: the ABI's declaration, export and refusals, the workspace size, the ground-truth lookup, the report's
format, the command lines' flags - and the near-tie colour set that lets the GPU test (tests/test_metrics_gpu.py) tell the model's luma from
an exact-integer and from an fp32 evaluation."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from PIL import Image

from tests.support import metrics_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


def test_header_declares_and_library_exports_the_entry_point():
    L, lib = _library()
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "int ir_metrics_y(ir_ctx* ctx, void* stream, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch" in header
    assert "IR_STAGE_METRICS = 12" in header
    assert "ir_metrics_y" in L.SYMBOLS and L.STAGE_METRICS == 12
    assert hasattr(lib, "ir_metrics_y")
    assert lib.ir_abi_version() == 3   # the entry point is additive
    from instarevive_amd import build
    assert "metrics.hip" in build.SOURCES


def test_workspace_needs_no_context():
    L, lib = _library()
    ws = lambda n, h, w: lib.ir_workspace_bytes(None, L.STAGE_METRICS, n, h, w, 0, 0, 0)
    for n, h, w in [(1, 11, 11), (1, 12, 75), (3, 139, 201), (1, 2048, 2048), (8, 512, 512)]:
        assert ws(n, h, w) > 0, (n, h, w)
    assert ws(0, 64, 64) == 0 and ws(1, 0, 64) == 0 and ws(1, 64, 0) == 0 and ws(-1, 64, 64) == 0
    assert ws(8, 2048, 2048) >= 8 * ws(1, 2048, 2048) - 8 * 256   # partial sums per image
    from instarevive_amd import metrics
    assert metrics.ws_bytes(2, 96, 80) == ws(2, 96, 80)


def test_call_refuses_a_null_context_and_bad_sizes():
    _, lib = _library()
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is launched
    call = lambda a, b, out, ws, n, h, w, rows=64, pitch=192, wsb=1 << 20: lib.ir_metrics_y(None, None, a, rows, pitch, b, rows, pitch, n, h, w, out, ws, wsb)
    assert call(fake, fake, fake, fake, 1, 64, 64) == -1        # the null context
    for n, h, w in [(0, 64, 64), (1, 10, 64), (1, 64, 10), (1, 65, 64), (1, 64, 65)]:
        assert call(fake, fake, fake, fake, n, h, w) == -1, (n, h, w)
    assert call(None, fake, fake, fake, 1, 64, 64) == -1 and call(fake, fake, None, fake, 1, 64, 64) == -1
    assert call(fake, fake, fake, fake, 1, 64, 64, wsb=0) == -1


def test_psnr_from_mse_is_the_models():
    from instarevive_amd.metrics import psnr_from_mse
    a, b = M.noise(16, 20, 1), M.noise(16, 20, 2)
    mse, psnr, _ = M.model_scores(a, b)
    assert psnr_from_mse(mse) == pytest.approx(psnr, abs=1e-12)
    assert psnr_from_mse(0.0) == pytest.approx(80.0, abs=1e-12)


def test_ground_truth_lookup(tmp_path):
    from instarevive_amd.metrics import GroundTruth, MetricsError
    inp, gt = tmp_path / "in", tmp_path / "gt"
    (inp / "deep").mkdir(parents=True)
    (gt / "deep").mkdir(parents=True)
    img = Image.fromarray(M.noise(12, 14, 0))
    for p in (inp / "a.png", inp / "deep" / "b.png", inp / "deep" / "c.jpg", inp / "deep" / "d.png", inp / "deep" / "e.png", gt / "a.JPG", gt / "deep" / "b.png",
              gt / "b.png", gt / "c.png", gt / "d.png", gt / "d.jpeg", gt / "notes.txt", gt / "e.txt"):
        if p.suffix == ".txt":
            p.write_text("x")
        else:
            img.save(p)
    look = GroundTruth(str(gt), str(inp))
    assert look.path(str(inp / "a.png")) == str(gt / "a.JPG")                 # any image extension, whatever its case
    assert look.path(str(inp / "deep" / "b.png")) == str(gt / "deep" / "b.png")   # the relative path first ...
    assert look.path(str(inp / "deep" / "c.jpg")) == str(gt / "c.png")        # ... then the flat folder by stem
    assert look.load(str(inp / "a.png")).size == (14, 12)
    with pytest.raises(MetricsError, match="ambiguous") as e:
        look.path(str(inp / "deep" / "d.png"))
    assert "d.png" in str(e.value)
    with pytest.raises(MetricsError, match="no ground truth") as e:
        look.path(str(inp / "deep" / "e.png"))                                # e.txt is no image
    assert str(inp / "deep" / "e.png") in str(e.value)
    assert GroundTruth(str(gt)).path(str(inp / "deep" / "b.png")) == str(gt / "b.png")   # without an input root: the stem alone
    with pytest.raises(MetricsError):
        GroundTruth(str(tmp_path / "none"))


def test_report_format_is_evaluate_pairs(tmp_path):
    from instarevive_amd.metrics import Report, read_report
    folder_a, folder_b = tmp_path / "a", tmp_path / "b"
    folder_a.mkdir()
    folder_b.mkdir()
    rep = Report(str(tmp_path / "out" / "metrics.csv"))
    for i in range(3):
        a, b = M.noise(16, 24, 10 + i), M.noise(16, 24, 20 + i)
        Image.fromarray(a).save(folder_a / f"im{i}.png")
        Image.fromarray(b).save(folder_b / f"im{i}.png")
        _, psnr, ssim = M.model_scores(a, b)
        rep.add(f"sub/im{2 - i},x.png" if i == 0 else f"im{i}.png", psnr, ssim)
    lines = []
    M.EP.evaluate(str(folder_a), str(folder_b), log=lines.append)
    assert rep.write() == lines[1:] and len(lines) == 3 and lines[1].startswith("psnr: ") and lines[2].startswith("ssim: ")
    text = (tmp_path / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,psnr_y,ssim_y" and len(text) == 4
    back = read_report(str(tmp_path / "out" / "metrics.csv"))
    assert back == {name: (p, s) for name, p, s in rep.rows}      # every digit survives, a comma in a name included
    assert Report().write() == []


def test_check_ground_truth_names_both_sizes():
    from instarevive_amd.metrics import check_ground_truth
    check_ground_truth([M.noise(12, 14, 0)], [(12, 14)])
    with pytest.raises(ValueError, match="12 x 14.*12 x 15"):
        check_ground_truth([M.noise(12, 14, 0)], [(12, 15)])
    with pytest.raises(ValueError):
        check_ground_truth([M.noise(12, 14, 0)], [(12, 14), (12, 14)])
    with pytest.raises(ValueError):
        check_ground_truth([M.noise(12, 14, 0).astype(np.float32)], [(12, 14)])
    with pytest.raises(ValueError, match="11 x 11"):
        check_ground_truth([M.noise(10, 14, 0)], [(10, 14)])


def test_command_lines_parse_gt(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"])
    assert inf.parse_args().gt is None and inf.parse_args().metrics_out is None and eval_batch.parse_args().gt is None
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--gt", "truth"])
    assert inf.parse_args().gt == "truth" and eval_batch.parse_args().gt == "truth"
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--gt", "truth", "--metrics_out", "m.csv"])
    assert inf.parse_args().metrics_out == "m.csv"
    monkeypatch.setattr(sys, "argv", ["evaluate_pairs.py", "-i", "a", "-r", "b", "--backend", "gpu"])
    seen = {}
    monkeypatch.setattr(M.EP, "evaluate", lambda *a, **k: seen.update(k))
    M.EP.main()
    assert seen["backend"] == "gpu"
    monkeypatch.setattr(sys, "argv", ["evaluate_pairs.py", "-i", "a", "-r", "b"])
    M.EP.main()
    assert seen["backend"] == "host"


def test_read_job_attaches_the_ground_truth_of_scored_jobs_only(tmp_path):
    sys.path.insert(0, ROOT)
    from argparse import Namespace
    import inference as inf
    from instarevive_amd.metrics import GroundTruth, MetricsError
    inp, gt = tmp_path / "in", tmp_path / "gt"
    inp.mkdir()
    gt.mkdir()
    Image.fromarray(M.noise(40, 56, 1)).save(inp / "small.png")     # auto_resize enlarges it: the host would resize the result back
    Image.fromarray(M.noise(520, 600, 2)).save(inp / "big.png")     # a plain crop
    Image.fromarray(M.noise(520, 600, 3)).save(inp / "odd.png")
    Image.fromarray(M.noise(40, 56, 4)).save(gt / "small.png")
    Image.fromarray(M.noise(520, 600, 5)).save(gt / "big.png")
    Image.fromarray(M.noise(520, 601, 6)).save(gt / "odd.png")
    base = dict(input=str(inp), output=str(tmp_path / "out"), sr_scale=1, tiled=False, tile_size=512, use_center_crop=False, show_lq=False,
                disable_preprocess_model=False, gt_lookup=GroundTruth(str(gt), str(inp)))
    args = Namespace(**base)
    assert inf.read_job(str(inp / "small.png"), 0, args).gt is None
    big = inf.read_job(str(inp / "big.png"), 0, args)
    assert big.gt.shape == (520, 600, 3) and np.array_equal(big.gt, M.noise(520, 600, 5))
    with pytest.raises(MetricsError, match="520 x 601.*520 x 600"):
        inf.read_job(str(inp / "odd.png"), 0, args)
    small = inf.read_job(str(inp / "small.png"), 0, Namespace(**dict(base, resize_on_gpu=True)))   # --resize gpu: the device's image is the saved one
    assert small.gt.shape == (40, 56, 3)
    assert inf.read_job(str(inp / "big.png"), 0, Namespace(**dict(base, show_lq=True))).gt is None
    assert inf.read_job(str(inp / "big.png"), 0, Namespace(**dict(base, gt_lookup=None))).gt is None


# ---------------------------------------------------------------------------------------------------------------- the near-tie colours
def test_near_tie_colours_separate_the_luma_variants():
    """The model divides in float32 before it widens: exact integer arithmetic rounds 80 of the 2^24 colours differently, an fp32 evaluation 123.
    On a 24 x 32 image drawn from them (partner: +-6 per sample) both variants must miss the model's SSIM by far more than the GPU test's
    tolerance - so a kernel that passes there has the model's luma."""
    exact, fp32 = M.near_tie_colours()
    assert len(exact) == 80 and len(fp32) == 123
    a, b = M.near_tie_pair()
    assert a.shape == (24, 32, 3)
    model = M.model_scores(a, b)[2]
    assert model == M.ssim_of_luma(M.luma_model(a), M.luma_model(b))
    d_exact = abs(model - M.ssim_of_luma(M.luma_exact(a), M.luma_exact(b)))
    d_fp32 = abs(model - M.ssim_of_luma(M.luma_fp32(a), M.luma_fp32(b)))
    print(f"near-tie pair: model ssim {model:.9f}, exact-integer luma off by {d_exact:.3e}, fp32 luma off by {d_fp32:.3e}")
    assert d_exact > 1e-7 and d_fp32 > 1e-7 and min(d_exact, d_fp32) > 100 * M.SSIM_TOL


def test_luma_tables_round_like_the_model_on_every_colour():
    """What api_image.cpp uploads: t_k[v] = c_k * (double)((float)v / 255.0f), summed as 16 + t_r + t_g + t_b. Over the near-tie colours and a sample
    of all colours the rounded luma must be the model's (the closest the model comes to a tie is 2.2e-7)."""
    x = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float64)
    tab = [c * x for c in (65.481, 128.553, 24.966)]
    exact, fp32 = M.near_tie_colours()
    cols = np.concatenate([exact, fp32, M.noise(256, 256, 7).reshape(-1, 3)])
    s = 16.0 + tab[0][cols[:, 0]] + tab[1][cols[:, 1]] + tab[2][cols[:, 2]]
    assert np.array_equal(np.round(s / 255.0 * 255.0), M.luma_model(cols[None])[0])
    assert np.array_equal(s / 255.0, M.EP.to_y(M._unit(cols[None]), 1.0)[0])
