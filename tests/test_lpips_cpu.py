"""ir_lpips and its host side without a GPU: the ABI's declaration, export and refusals, the workspace size, the scaling table, the weight
loader, the report's optional column, the command lines' flags - and the float64 model of tests/support/lpips_model.py with the planted bugs
that show what the gate of the GPU test (tests/test_lpips_gpu.py) can tell apart."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import lpips_model as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_lpips():
    from instarevive_amd import build
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    lib = L.load_library()
    assert "int ir_lpips(ir_ctx* ctx, void* stream, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h," in header
    assert "int ir_lpips_configure(ir_ctx* ctx);" in header and "int ir_lpips_scale_table(float* tab768);" in header
    assert "IR_STAGE_LPIPS = 13" in header and L.STAGE_LPIPS == 13
    for name in ("ir_lpips", "ir_lpips_configure", "ir_lpips_scale_table"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.ir_abi_version() == 3
    assert "lpips.hip" in build.SOURCES


def _edge(e, k, s, p):
    return (e + 2 * p - k) // s + 1


def _expected_workspace(n, h, w):
    """Two ping-pong fp32 maps for the 2n images - conv1 / conv2 / conv3 / conv5 outputs share one, pool1 / pool2 / conv4 outputs the other -
    and one double per 64 output pixels of every stage and pair; each part rounded up to 256 bytes."""
    def up(v):
        return (v + 255) & ~255
    e = lambda x: _edge(x, 11, 4, 2)
    h1, w1 = e(h), e(w)
    hp1, wp1 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    hp2, wp2 = (hp1 - 3) // 2 + 1, (wp1 - 3) // 2 + 1
    x = max(h1 * w1 * 64, hp1 * wp1 * 192, hp2 * wp2 * 384, hp2 * wp2 * 256)
    y = max(hp1 * wp1 * 64, hp2 * wp2 * 192, hp2 * wp2 * 256)
    chunks = -(-h1 * w1 // 64) + -(-hp1 * wp1 // 64) + 3 * -(-hp2 * wp2 // 64)
    return up(2 * n * x * 4) + up(2 * n * y * 4) + up(n * chunks * 8)


def test_workspace_is_a_function_of_the_sizes_alone():
    from instarevive_amd import lpips
    ws = lambda n, h, w: L.load_library().ir_workspace_bytes(None, L.STAGE_LPIPS, n, h, w, 0, 0, 0)
    for n, h, w in [(1, 31, 31), (3, 35, 67), (4, 512, 512), (1, 2048, 2048), (2, 97, 130)]:
        assert ws(n, h, w) == _expected_workspace(n, h, w) == lpips.ws_bytes(n, h, w)
    assert ws(1, 30, 64) == 0 and ws(1, 64, 30) == 0 and ws(0, 64, 64) == 0
    assert 160e6 < ws(1, 2048, 2048) < 170e6   # the figure the header states


def test_refusals_need_no_gpu():
    """Every refusal is decided before anything touches the device: with a null context the call returns -1 for each."""
    lib = L.load_library()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    call = lambda a=p, b=p, out=p, ws=p, n=1, h=31, w=31, rows=31, pitch=93, wsb=1 << 20: lib.ir_lpips(None, None, a, rows, pitch, b, rows, pitch, n, h, w, out, ws, wsb)
    assert call() == -1                                                  # null context
    assert call(a=None) == -1 and call(n=0) == -1 and call(h=30) == -1 and call(rows=30) == -1 and call(pitch=92) == -1 and call(wsb=0) == -1
    assert lib.ir_lpips_configure(None) < 0 and lib.ir_lpips_scale_table(None) == -1


def test_scaling_table_is_the_torch_preprocessing_to_the_bit():
    """All 256 x 3 entries against the fp32 torch expressions of evaluate_pairs.LPIPS.__call__: v / 255, 2 x - 1, (x - shift) / scale."""
    from instarevive_amd.lpips import scaling_table
    tab = scaling_table()
    v = torch.arange(256, dtype=torch.float32).view(1, 1, 1, 256).expand(1, 3, 1, 256) / 255.0
    x = 2 * v - 1
    want = ((x - torch.tensor(LM.SHIFT).view(1, 3, 1, 1)) / torch.tensor(LM.SCALE).view(1, 3, 1, 1))[0, :, 0].numpy()
    assert tab.dtype == np.float32 and tab.shape == (3, 256)
    assert np.array_equal(tab.view(np.int32), want.view(np.int32))
    # and against what the float64 model feeds its first conv
    img = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1)[None]
    assert np.array_equal(LM.scaled_input(img)[0, :, 0].numpy().view(np.int32), tab.view(np.int32))


def test_float64_model_agrees_with_the_host_model():
    """fp32 rounding is 6e-8 per operation; a dot product of K <= 3456 terms accumulates about sqrt(K) of them (3.5e-6 worst per element, far less
    in the mean over a map): the host model must sit within 1e-5 of the float64 restatement on every case, or one of the two is not the model."""
    for name, *_ in LM.CASES:
        d = LM.host_deviation(name)
        print(f"{name}: float64 {LM.reference(name):.12g}, host fp32 off by {d:.3e}")
        assert d < 1e-5, (name, d)
    print(f"pooled {LM.pooled_host_deviation():.3e}, gate {LM.gate():.3e}")
    assert LM.gate() == 8 * max(LM.host_deviation(c[0]) for c in LM.CASES)
    assert LM.lpips_f64(LM.pair("31x31_noise")[0], LM.pair("31x31_noise")[0], LM.weights()) == 0.0


@pytest.mark.parametrize("bug", LM.PLANTED_BUGS)
def test_planted_bugs_land_outside_the_gate(bug):
    """Each known way to get AlexNet / LPIPS wrong, applied to the float64 model, must miss the gate by 1.5 x on at least one of the small cases."""
    gate = LM.gate()
    effect = {n: LM.rel(LM.lpips_f64(*LM.pair(n), LM.case_weights(n), bug), LM.reference(n)) for n in LM.SMALL}
    print(bug, {k: f"{v:.2e}" for k, v in effect.items()}, f"gate {gate:.2e}")
    assert max(effect.values()) >= 1.5 * gate, (bug, effect, gate)
    if bug == "ceil_pool":   # shows on the one case whose pool input is even, and nowhere else
        assert effect["35x67_noise"] >= 1.5 * gate and all(v == 0.0 for k, v in effect.items() if k != "35x67_noise")


def test_bf16_operands_would_miss_the_gate():
    """The gate is what rules bf16 MFMA operands out: conv1's weights alone rounded to bf16 move a small case by more than 1.5 x the gate."""
    w = dict(LM.weights())
    w["lpips.c1.w"] = w["lpips.c1.w"].bfloat16().float()
    effect = max(LM.rel(LM.lpips_f64(*LM.pair(n), w), LM.reference(n)) for n in ("31x31_noise", "34x31_pm6", "64x64_near"))
    assert effect >= 1.5 * LM.gate(), effect


def test_weight_loader_takes_both_file_forms_and_raises_the_models_errors(tmp_path):
    from instarevive_amd.lpips import load_weights
    w = LM.weights()
    alex, lin = LM.state_dicts(w)
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "lin.pth")
    _, full = LM.state_dicts(w, full=True)
    torch.save({"state_dict": full}, tmp_path / "full.pth")
    for got in (load_weights(str(tmp_path / "lin.pth"), str(tmp_path / "alexnet.pth")), load_weights(str(tmp_path / "full.pth")), load_weights(lin, alex)):
        assert sorted(got) == sorted(w)
        for k in w:
            assert got[k].dtype == torch.float32 and got[k].is_contiguous() and torch.equal(got[k], w[k]), k
    with pytest.raises(KeyError, match="AlexNet conv 1"):
        load_weights(str(tmp_path / "lin.pth"))
    with pytest.raises(KeyError, match="lin0.model.1.weight missing"):
        load_weights(None, str(tmp_path / "alexnet.pth"))
    bad = dict(lin)
    bad["lin2.model.1.weight"] = bad["lin2.model.1.weight"][:, :-1]
    with pytest.raises(ValueError, match="stage 2"):
        load_weights(bad, alex)
    # the same errors as the host model's constructor
    for args in ((None, lin), (alex, None), (alex, bad)):
        with pytest.raises((KeyError, ValueError)) as host:
            LM.EP.LPIPS(*args)
        with pytest.raises(type(host.value)) as ours:
            load_weights(args[1], args[0])
        assert str(ours.value) == str(host.value)


def test_report_carries_the_third_column_only_when_asked(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    plain = Report(str(tmp_path / "plain.csv"))
    plain.add("a.png", 30.5, 0.9)
    assert plain.write() == ["psnr: 30.50000", "ssim: 0.90000"]
    assert (tmp_path / "plain.csv").read_text().splitlines() == ["file,psnr_y,ssim_y", "a.png,30.5,0.9"]
    assert read_report(str(tmp_path / "plain.csv")) == {"a.png": (30.5, 0.9)} and plain.rows == [("a.png", 30.5, 0.9)]
    with pytest.raises(MetricsError):
        plain.add("b.png", 30.5, 0.9, 0.1)
    rep = Report(str(tmp_path / "three.csv"), lpips=True)
    rep.add("b,x.png", 31.25, 0.75, 0.123456789012345678)
    rep.add("a.png", 29.25, 0.25, 0.5)
    assert rep.write() == ["psnr: 30.25000", "ssim: 0.50000", f"lpips: {(0.123456789012345678 + 0.5) / 2:.5f}"]
    text = (tmp_path / "three.csv").read_text().splitlines()
    assert text[0] == "file,psnr_y,ssim_y,lpips" and len(text) == 3 and text[1].startswith("a.png,")
    assert read_report(str(tmp_path / "three.csv")) == {"b,x.png": (31.25, 0.75, 0.123456789012345678), "a.png": (29.25, 0.25, 0.5)}
    with pytest.raises(MetricsError):
        rep.add("c.png", 30.0, 0.5)
    assert Report(lpips=True).write() == []


def test_score_slot_and_ground_truth_check_know_the_31_pixel_edge():
    from instarevive_amd.metrics import check_ground_truth
    g = LM.noise(30, 100, 0)
    check_ground_truth([g], [(30, 100)])
    with pytest.raises(ValueError, match="31 x 31"):
        check_ground_truth([g], [(30, 100)], min_edge=31)
    check_ground_truth([LM.noise(31, 31, 0)], [(31, 31)], min_edge=31)


def test_command_lines_parse_lpips_flags(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    assert inf.parse_args().lpips_lin is None and inf.parse_args().lpips_alexnet is None and eval_batch.parse_args().lpips_lin is None
    monkeypatch.setattr(sys, "argv", base + ["--gt", "t", "--lpips_lin", "lin.pth", "--lpips_alexnet", "alex.pth"])
    for mod in (inf, eval_batch):
        a = mod.parse_args()
        assert (a.gt, a.lpips_lin, a.lpips_alexnet) == ("t", "lin.pth", "alex.pth")
    # evaluate_pairs --backend gpu with weights takes LPIPS from the device; --backend host keeps the torch model
    seen = {}
    monkeypatch.setattr(LM.EP, "evaluate", lambda *a, **k: seen.update(k))
    monkeypatch.setattr(LM.EP, "_gpu_lpips", lambda alexnet, lin: ("device", alexnet, lin))
    monkeypatch.setattr(LM.EP, "LPIPS", lambda alexnet, lin, device: ("host", alexnet, lin))
    monkeypatch.setattr(sys, "argv", ["evaluate_pairs.py", "-i", "a", "-r", "b", "--backend", "gpu", "--lpips_lin", "lin.pth"])
    LM.EP.main()
    assert seen["backend"] == "gpu" and seen["lpips_u8"] == ("device", None, "lin.pth") and seen.get("lpips") is None
    seen.clear()
    monkeypatch.setattr(sys, "argv", ["evaluate_pairs.py", "-i", "a", "-r", "b", "--lpips_lin", "lin.pth", "--lpips_alexnet", "alex.pth"])
    LM.EP.main()
    assert seen["backend"] == "host" and seen["lpips"] == ("host", "alex.pth", "lin.pth") and "lpips_u8" not in seen


def test_lpips_without_gt_is_refused_before_any_model_is_touched():
    from instarevive_amd.pipeline import process, process_stream
    img = [LM.noise(64, 64, 0)]
    with pytest.raises(ValueError, match="lpips.*gt"):
        process(None, img, 1, "wavelet", False, False, 64, 32, lpips=True)
    with pytest.raises(ValueError, match="lpips.*gt"):
        next(process_stream(None, [img], "wavelet", False, False, 64, 32, lpips=True))
