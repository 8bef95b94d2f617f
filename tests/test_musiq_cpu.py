"""MUSIQ without a GPU: the definition (tools/evaluate_musiq.py) against its own planted bugs and against pyiqa's padded form, the library's host
answers (ir_musiq_layout, ir_musiq_input_table) against the model, the loader, the report's columns and the command lines."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.support import musiq_model as MM

EM = MM.EM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the definition and its gate
def test_gate_yardsticks():
    """The gate comes from the host model alone: 8 x the fp32 CPU model's largest deviation from the float64 model over the cases."""
    for name, h, w, _ in MM.CASES:
        print(f"{name:12s} T {EM.layout(h, w)[2]:4d} score {MM.reference(name)[0]:+.6f} host deviation: score {MM.host_deviation(name)[0]:.3e} feature {MM.host_deviation(name)[1]:.3e}")
    gs, gf = MM.gate()
    print(f"gate: score {gs:.3e} feature {gf:.3e}")
    assert 0 < gs < 1e-3 and 0 < gf < 1e-3   # an fp32 model of this depth: far below a bf16 operand's 4e-3
    assert [EM.layout(h, w)[2] for _, h, w, _ in MM.CASES[:3]] == [195, 107, 109] and EM.layout(300, 500)[2] == 292 and EM.layout(2048, 2048)[2] == 4290
    assert len({MM.reference(n)[0] for n, *_ in MM.CASES}) == len(MM.CASES)


def test_every_planted_bug_misses_the_gate_tenfold():
    """One wrong step each (evaluate_musiq.VARIANTS), in float64, over the small cases: the larger of score deviation / score gate and feature
    deviation / feature gate, per case. Every bug exceeds 10 on at least one case. The rounding bug can only show where h * ratio ends in .5,
    which no case does: the table carries MM.ROUNDING_CASE for it in addition (the gate does not)."""
    gs, gf = MM.gate()
    names = MM.SMALL + (MM.ROUNDING_CASE[0],)
    print("bug".ljust(22) + "".join(n.rjust(11) for n in names))
    failed = []
    for bug in MM.PLANTED_BUGS:
        ratios = []
        for n in names:
            ds, df = MM.deviations(*MM.run(n, variant=bug), n)
            ratios.append(max(ds / gs, df / gf))
        print(bug.ljust(22) + "".join(f"{r:11.3g}" for r in ratios))
        if max(ratios) <= 10:
            failed.append(bug)
    assert len(MM.PLANTED_BUGS) == 13 and not failed, failed


def test_dropping_the_masked_padding_tokens_changes_nothing():
    """pyiqa pads the resized scales to 49 / 144 tokens and masks them with -1e3; the model leaves them out. Both forms of the float64 model."""
    for n in MM.SMALL:
        score, feat = MM.run(n, padding="masked")
        rs, rf = MM.reference(n)
        assert abs(score - rs) <= 1e-12 and np.abs(feat - rf).max() <= 1e-12, n
    x = EM.scaled_input(MM.image("33x70")).double()
    assert EM.patches_of(x, padding="masked")[0].shape[0] == 49 + 144 + 6 and EM.patches_of(x)[0].shape[0] == 106


def test_written_out_bicubic_is_torchs():
    x = torch.randn(1, 3, 13, 21, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for rh, rw in ((30, 17), (7, 9), (13, 21), (1, 40)):
        assert (EM.bicubic(x, rh, rw) - EM.resize(x, rh, rw)).abs().max() <= 1e-13
    assert (EM.bicubic(x, 30, 17, -0.5) - EM.resize(x, 30, 17)).abs().max() > 1e-3


# ---------------------------------------------------------------------------------------------------------------- the library's host answers
def _same_layout(h, w):
    from instarevive_amd import musiq
    got = musiq.layout(h, w)
    try:
        scales, index, T = EM.layout(h, w)
    except EM.MusiqError:
        return got is None and not musiq.scorable(h, w)
    return got is not None and got[0] == T and got[1] == [tuple(s) for s in scales] and np.array_equal(got[2], index.numpy()) and musiq.scorable(h, w)


def test_library_layout_is_the_models():
    from instarevive_amd import _lib, musiq
    from instarevive_amd.build import build
    build()
    for h in range(1, 131):
        for w in range(1, 131):
            assert _same_layout(h, w), (h, w)
    # large and extreme sizes, and sizes where h * ratio ends in .5 (224 / 448 and 384 / 768 halve an odd side)
    for h, w in ((2048, 2048), (223, 224), (224, 223), (3, 64), (64, 3), (35, 448), (448, 35), (101, 768), (768, 5), (1, 300), (2047, 1366), (1, 1), (4096, 31)):
        assert _same_layout(h, w), (h, w)
    assert musiq.layout(2048, 2048)[0] == 4290 and musiq.layout(32, 32)[0] == 195
    assert musiq.layout(1, 1000) is None and musiq.layout(1000, 1) is None and musiq.layout(0, 5) is None
    with pytest.raises(EM.MusiqError, match="1 x 1000"):
        EM.layout(1, 1000)
    lib = _lib.load_library()
    lon = (C.c_int * 3)(*_lib.MUSIQ_LONGER)
    idx = (C.c_int * 4)()
    assert lib.ir_musiq_layout(32, 32, 32, 10, 3, lon, None, idx, 4) == -1      # cap below T - 1
    assert lib.ir_musiq_layout(32, 32, 32, 10, 5, lon, None, None, 0) == -1     # more scales than the library takes
    assert lib.ir_workspace_bytes(None, _lib.STAGE_MUSIQ, 1, 64, 64, 0, 0, 0) == 0   # no context, nothing configured


def test_library_table_is_torchs_roundings():
    from instarevive_amd import musiq
    from instarevive_amd.build import build
    build()
    tab = musiq.input_table()
    assert tab.dtype == np.float32 and np.array_equal(tab, EM.input_table())
    assert tab[0] == -1.0 and tab[255] == 1.0 and np.all(np.diff(tab) > 0)


def test_header_symbols_and_build_list_move_together():
    from instarevive_amd import _lib
    from instarevive_amd.build import FILE_FLAGS, SOURCES
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    for s in ("ir_musiq_layout", "ir_musiq_input_table", "ir_musiq_configure", "ir_musiq"):
        assert s in _lib.SYMBOLS and f"int {s}(" in header
    assert "IR_STAGE_MUSIQ = 21" in header and _lib.STAGE_MUSIQ == 21 and _lib.MUSIQ_NOT_CONFIGURED == -13
    assert "musiq.hip" in SOURCES and FILE_FLAGS["musiq.hip"] == ["-ffp-contract=off"]


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_loader_round_trips_an_npz_and_a_pth(tmp_path):
    from instarevive_amd import musiq
    m = MM.model("small")
    EM.save_npz(tmp_path / "m.npz", m)
    got = musiq.load_model(str(tmp_path / "m.npz"))
    assert got["cfg"] == m["cfg"] and got["cfg"]["layers"] == 2 and set(got["sd"]) == set(m["sd"])
    assert all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"]) and all(torch.equal(got["std"][k], m["std"][k]) for k in EM.CONVS)
    # the standardised weights: zero mean per output channel, and the stated formula
    w = m["sd"]["block.conv2.weight"].double()
    want = (w - w.mean((1, 2, 3), keepdim=True)) / torch.sqrt(w.var((1, 2, 3), unbiased=False, keepdim=True) + 1e-5)
    assert torch.equal(m["std"]["block.conv2"], want.float()) and m["std"]["block.conv2"].dtype == torch.float32
    # a .pth through the recalled name table, plain and wrapped; the embeddings in pyiqa's [1][rows][hidden] form
    keys = EM.PYIQA_KEYS(2)
    assert set(keys) == set(m["sd"])
    pth = {keys[k]: (v[None] if k in ("position_emb", "scale_emb") else v.reshape(1, 1, -1) if k == "cls_token" else v) for k, v in m["sd"].items()}
    torch.save(pth, tmp_path / "plain.pth")
    torch.save({"params": pth}, tmp_path / "wrapped.pth")
    for f in ("plain.pth", "wrapped.pth"):
        got = EM.load_model(str(tmp_path / f))
        assert got["cfg"] == m["cfg"] and all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"])
    bad = {k: v.numpy() for k, v in m["sd"].items()}
    del bad["layers.1.attn.k.bias"]
    np.savez(tmp_path / "missing.npz", **bad)
    with pytest.raises(EM.MusiqError, match=r"missing\.npz: layers\.1\.attn\.k\.bias missing"):
        EM.load_model(str(tmp_path / "missing.npz"))
    bad = {k: v.numpy() for k, v in m["sd"].items()}
    bad["scale_emb"] = bad["scale_emb"][:2]
    np.savez(tmp_path / "shape.npz", **bad)
    with pytest.raises(EM.MusiqError, match=r"scale_emb is \(2, 384\)"):
        EM.load_model(str(tmp_path / "shape.npz"))
    assert musiq.MusiqError is EM.MusiqError and issubclass(EM.MusiqError, ValueError)


# ---------------------------------------------------------------------------------------------------------------- report and command lines
def test_report_columns_and_the_unscored_order(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    values = dict(psnr=30.5, ssim=0.9, lpips=0.25, niqe=6.5, clipiqa=0.625, musiq=61.25)
    for paired in (True, False):
        for lp in (False, True):
            for nq in (False, True):
                for cq in (False, True):
                    for mq in (False, True):
                        if not paired and (lp or not (nq or cq or mq)):
                            with pytest.raises(MetricsError):
                                Report(None, lpips=lp, niqe=nq, paired=paired, clipiqa=cq, musiq=mq)
                            continue
                        keys = ((("psnr", "ssim") if paired else ()) + (("lpips",) if lp else ()) + (("niqe",) if nq else ()) + (("clipiqa",) if cq else ())
                                + (("musiq",) if mq else ()))
                        path = tmp_path / f"r{paired:d}{lp:d}{nq:d}{cq:d}{mq:d}.csv"
                        rep = Report(str(path), lpips=lp, niqe=nq, paired=paired, clipiqa=cq, musiq=mq)
                        rep.add_scores("b.png", tuple(values[k] for k in keys))
                        rep.add("a.png", **{k: values[k] + 1 for k in keys})
                        assert rep.write() == [f"{k}: {values[k] + 0.5:.5f}" for k in keys]
                        header = ",".join(("file",) + tuple({"psnr": "psnr_y", "ssim": "ssim_y"}.get(k, k) for k in keys))
                        assert path.read_text().splitlines()[0] == header and header in Report.HEADERS
                        assert read_report(str(path)) == {"b.png": tuple(values[k] for k in keys), "a.png": tuple(values[k] + 1 for k in keys)}
                        if not mq:
                            with pytest.raises(MetricsError):
                                rep.add("x", **{k: values[k] for k in keys}, musiq=0.5)
    assert Report(None, lpips=True, niqe=True, clipiqa=True, musiq=True).header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq"
    assert Report(None, musiq=True, paired=False).header() == "file,musiq" and Report(None, musiq=True).header() == "file,psnr_y,ssim_y,musiq"
    assert len(Report.HEADERS) == len(set(Report.HEADERS)) == 23
    nan = float("nan")
    full = Report(None, lpips=True, niqe=True, clipiqa=True, musiq=True)
    assert full.unscored((30.0, 0.9, 0.1, 4.0, 0.5, 60.0)) is None and full.unscored((30.0, 0.9, 0.1, 4.0, 0.5, nan)) == "musiq"
    assert full.unscored((30.0, 0.9, 0.1, 4.0, nan, nan)) == "clipiqa" and full.unscored((30.0, 0.9, 0.1, nan, 0.5, nan)) == "niqe"   # musiq is looked at last
    assert Report(None, musiq=True, paired=False).unscored((nan,)) == "musiq"


def test_command_lines_parse_and_refuse_a_bad_model_file(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    assert inf.parse_args().musiq_model is None and eval_batch.parse_args().musiq_model is None
    assert inf.load_musiq_model(inf.parse_args()) is None
    missing = str(tmp_path / "nowhere.npz")
    monkeypatch.setattr(sys, "argv", base + ["--musiq_model", missing])
    assert inf.parse_args().musiq_model == missing and eval_batch.parse_args().musiq_model == missing
    # refused before any model is touched: neither the device check nor the loaders run
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match="nowhere.npz"):
            main()
    m = MM.model("small")
    part = {k: v.numpy() for k, v in m["sd"].items() if k != "head.bias"}
    np.savez(tmp_path / "part.npz", **part)
    monkeypatch.setattr(sys, "argv", base + ["--musiq_model", str(tmp_path / "part.npz")])
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match=r"part\.npz.*head\.bias missing"):
            main()
    assert touched == []
    EM.save_npz(tmp_path / "good.npz", m)
    # the conflict of every scored run names the flag: the tile-sharded path is not scored on the device (refused once the models are loaded)
    assert "--gt / --niqe_params / --clipiqa_model / --musiq_model are not offered together with --shard_tiles" in open(os.path.join(ROOT, "inference.py")).read()
    monkeypatch.setattr(sys, "argv", base + ["--musiq_model", str(tmp_path / "good.npz")])
    got = inf.load_musiq_model(inf.parse_args())
    assert got["cfg"]["layers"] == 2 and got["cfg"]["hidden"] == 384
    monkeypatch.setattr(sys, "argv", ["evaluate_musiq.py", "-i", "a", "--musiq_model", "m.npz", "--backend", "gpu", "--ntest", "3"])
    seen = {}
    monkeypatch.setattr(EM, "evaluate", lambda *a, **k: seen.update(k, args=a))
    EM.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "m.npz", 3)


def test_evaluate_musiq_averages_a_folder(tmp_path):
    from PIL import Image
    EM.save_npz(tmp_path / "m.npz", MM.model("small"))
    for name in ("32x32", "33x70"):
        Image.fromarray(MM.image(name)).save(tmp_path / f"{name}.png")
    Image.fromarray(MM.ramp(1, 1000, 1)).save(tmp_path / "sliver.png")
    lines = []
    avg = EM.evaluate(str(tmp_path), str(tmp_path / "m.npz"), log=lines.append)
    want = (MM.reference("32x32")[0] + MM.reference("33x70")[0]) / 2
    assert abs(avg - want) <= MM.gate()[0] and lines[-1] == f"musiq: {avg:.5f}" and "1 not scored" in lines[-2]
