"""tools/evaluate_maniqa.py, the definition ir_maniqa is tested against, and the host parts of the MANIQA scorer: no GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.support import maniqa_model as MM

EM = MM.EM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_heads_of_the_seeded_models_are_alive():
    """The condition on the seeded weights, on the reference alone: more than half of the per-patch scores above 0 and every weight inside
    (0.02, 0.98) on every case - a dead head would let any trunk pass."""
    for name in (c[0] for c in MM.CASES):
        score, _, (s, w) = MM.reference(name)
        print(f"{name}: maniqa {score:.9f}; {np.mean(s > 0):.3f} of the scores above 0, weights within {w.min():.3f} .. {w.max():.3f}")
        assert np.isfinite(score) and np.mean(s > 0) > 0.5 and 0.02 < w.min() and w.max() < 0.98


def test_gate_yardsticks():
    ds, df = MM.pooled_host_deviation()
    gs, gf = MM.gate()
    for name in (c[0] for c in MM.CASES):
        print(f"{name}: host fp32 deviation {MM.host_deviation(name)[0]:.3e} (score), {MM.host_deviation(name)[1]:.3e} (tokens)")
    print(f"gate: {gs:.3e} (score), {gf:.3e} (tokens)")
    assert 0 < ds and 0 < df and gs == MM.GATE_FACTOR * ds and gf == MM.GATE_FACTOR * df and MM.GATE_FACTOR == 8.0


def test_every_planted_bug_misses_the_gate_tenfold():
    gs, gf = MM.gate()
    assert len(MM.PLANTED_BUGS) >= 12
    for v in MM.PLANTED_BUGS:
        worst = 0.0
        for name in MM.SMALL:
            s, f, _ = MM.run(name, torch.float64, v)
            ds, df = MM.deviations(s, f, name)
            worst = max(worst, ds / gs, df / gf)
        print(f"{v}: misses the gate {worst:.1f} times")
        assert worst > 10.0, v


# ---------------------------------------------------------------------------------------------------------------- crops
def test_crop_origins_by_hand_and_through_the_library():
    from instarevive_amd import maniqa
    from instarevive_amd.build import build
    build()
    assert EM.crop_origins(65, 65, 64, 5) == [(0, 0)] * 5                                            # step 1 // 2 = 0
    assert EM.crop_origins(70, 131, 64, 5) == [(0, 0), (0, 33), (0, 66), (3, 0), (3, 33)]            # steps 6 // 2, 67 // 2; a 3 x 3 grid, the first 5
    got = EM.crop_origins(100, 200, 64, 20)                                                          # steps 36 // 4, 136 // 4; a 5 x 5 grid, the first 20
    assert got == [(9 * i, 34 * j) for i in range(5) for j in range(5)][:20] and got[-1] == (27, 136)
    assert EM.crop_origins(300, 500, 224, 1) == [(0, 0)] and EM.crop_origins(300, 500, 224, 4) == [(0, 0), (0, 138), (38, 0), (38, 138)]
    for h, w, crop, crops in ((65, 65, 64, 5), (70, 131, 64, 5), (100, 200, 64, 20), (512, 512, 224, 20), (2048, 1000, 224, 20), (225, 300, 224, 1), (99, 77, 64, 17)):
        org = EM.crop_origins(h, w, crop, crops)
        assert maniqa.crop_origins(h, w, crop, crops) == org and len(org) == crops
        EM.check_origins(h, w, crop, org)
    for h, w in ((64, 200), (200, 64), (10, 10)):
        assert not maniqa.scorable(h, w, 64)
        with pytest.raises(EM.ManiqaError, match=f"{h} x {w}"):
            EM.crop_origins(h, w, 64, 5)
        with pytest.raises(EM.ManiqaError):
            maniqa.crop_origins(h, w, 64, 5)
    out = (C.c_int * 2)()
    lib = maniqa.L.load_library()
    assert lib.ir_maniqa_crops(65, 65, 64, 0, out) == -1 and lib.ir_maniqa_crops(64, 65, 64, 1, out) == -1 and lib.ir_maniqa_crops(65, 65, 64, 1, out) == 0
    # random: inside the image, a function of (seed, name) alone, the default seed stated
    a = EM.crop_origins(97, 83, 64, 5, "random", 7, "a.png")
    assert a == maniqa.crop_origins(97, 83, 64, 5, "random", 7, "a.png") and a != EM.crop_origins(97, 83, 64, 5, "random", 7, "b.png")
    assert a != EM.crop_origins(97, 83, 64, 5, "random", 8, "a.png") and len(set(a)) > 1
    assert EM.crop_origins(97, 83, 64, 5, "random", None, "a.png") == EM.crop_origins(97, 83, 64, 5, "random", EM.DEFAULT_SEED, "a.png")
    EM.check_origins(97, 83, 64, a)
    for bad in ((34, 0), (0, 20), (-1, 0)):
        with pytest.raises(EM.ManiqaError, match="origin"):
            EM.check_origins(97, 83, 64, [bad])


# ---------------------------------------------------------------------------------------------------------------- the model's parts
def test_tab_reinterpretation_is_the_literal_expression():
    g = torch.Generator().manual_seed(3)
    B, Cc, N = 2, 12, 5
    p = torch.randn((B, Cc, N), generator=g, dtype=torch.float64)
    lit = p.transpose(1, 2).reshape(B, Cc, N)
    for b in range(B):
        got = EM.tab_reinterpret(p[b])
        assert torch.equal(got, lit[b])
        flat = got.reshape(-1)
        assert all(flat[n * Cc + c] == p[b, c, n] for c in range(Cc) for n in range(N))
    assert not torch.equal(lit, p)
    # the whole block against the published forward written out
    sd = {f"t.{n}.{v}": torch.randn((N, N) if v == "weight" else (N,), generator=g, dtype=torch.float64) for n in "qkv" for v in ("weight", "bias")}
    x = torch.randn((B, Cc, N), generator=g, dtype=torch.float64)
    q, k, v = (x @ sd[f"t.{n}.weight"].t() + sd[f"t.{n}.bias"] for n in "qkv")
    attn = torch.softmax(q @ k.transpose(-2, -1) * N ** -0.5, dim=-1)
    want = (attn @ v).transpose(1, 2).reshape(B, Cc, N) + x
    assert torch.allclose(EM.tab(x, sd, "t"), want, rtol=0, atol=1e-12)


def test_shift_mask_and_relative_position_index_by_brute_force():
    for ws in (2, 4):
        idx = EM.relative_position_index(ws)
        for i in range(ws * ws):
            for j in range(ws * ws):
                dy, dx = i // ws - j // ws, i % ws - j % ws
                assert idx[i, j] == (dy + ws - 1) * (2 * ws - 1) + dx + ws - 1
        assert torch.equal(EM.relative_position_index(ws, True), idx.t()) and not torch.equal(idx, idx.t())
    for G, ws in ((8, 4), (28, 4), (12, 2)):
        shift = ws // 2
        m = EM.shift_mask(G, ws, shift)
        nw = G // ws
        assert m.shape == (nw * nw, ws * ws, ws * ws)

        def label(v):   # of a coordinate of the SHIFTED map
            return 0 if v < G - ws else 1 if v < G - shift else 2

        kinds = set()
        for wy in range(nw):
            for wx in range(nw):
                labs = [3 * label(wy * ws + i // ws) + label(wx * ws + i % ws) for i in range(ws * ws)]
                kinds.add(len(set(labs)))
                for i in range(ws * ws):
                    for j in range(ws * ws):
                        assert m[wy * nw + wx, i, j] == (0.0 if labs[i] == labs[j] else EM.MASK)
        assert kinds == {1, 2, 4}   # unmasked windows, windows cut along one axis, the corner window cut along both
    assert EM.MASK == -100.0


def test_library_table_is_torchs_roundings():
    from instarevive_amd import maniqa
    from instarevive_amd.build import build
    build()
    tab = maniqa.input_table()
    assert tab.dtype == np.float32 and np.array_equal(tab, EM.input_table())
    assert tab[0] == -1.0 and tab[255] == 1.0 and np.all(np.diff(tab) > 0)


def test_header_symbols_and_build_list_move_together():
    from instarevive_amd import _lib
    from instarevive_amd.build import FILE_FLAGS, SOURCES
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    for s in ("ir_maniqa_input_table", "ir_maniqa_crops", "ir_maniqa_configure", "ir_maniqa"):
        assert s in _lib.SYMBOLS and f"int {s}(" in header
    assert "IR_STAGE_MANIQA = 22" in header and _lib.STAGE_MANIQA == 22 and _lib.MANIQA_NOT_CONFIGURED == -13
    assert "maniqa.hip" in SOURCES and FILE_FLAGS["maniqa.hip"] == ["-ffp-contract=off"]


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_loader_round_trips_an_npz_and_a_pth(tmp_path):
    from instarevive_amd import maniqa
    m = MM.model("small")
    EM.save_npz(tmp_path / "m.npz", m)
    got = maniqa.load_model(str(tmp_path / "m.npz"))
    assert got["cfg"] == m["cfg"] and got["cfg"]["taps"] == (1, 2, 3, 4) and got["cfg"]["crops"] == 5 and set(got["sd"]) == set(m["sd"]) == set(EM.model_keys(m["cfg"]))
    assert all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"])
    # a .pth through the recalled name table, plain and wrapped, in timm's shapes, with ViT blocks behind the last tap and Swin's buffers present
    keys = EM.PYIQA_KEYS(m["cfg"])
    assert set(keys) == set(m["sd"])
    pth = {keys[k]: (v[None] if k == "vit.pos_embed" else v.reshape(1, 1, -1) if k == "vit.cls_token" else v[:, :, None, None] if k in ("conv1.weight", "conv2.weight") else v)
           for k, v in m["sd"].items()}
    for k in list(pth):
        if k.startswith("vit.blocks.4."):
            pth[k.replace("vit.blocks.4.", "vit.blocks.5.")] = pth[k] + 1
    pth["vit.norm.weight"], pth["vit.head.weight"] = torch.ones(64), torch.ones(10, 64)
    pth["swintransformer1.layers.0.blocks.1.attn_mask"] = torch.zeros(4, 16, 16)
    pth["swintransformer1.layers.0.blocks.0.attn.relative_position_index"] = torch.zeros(16, 16)
    torch.save(pth, tmp_path / "plain.pth")
    torch.save({"params": pth}, tmp_path / "wrapped.pth")
    given = {k: m["cfg"][k] for k in ("taps", "scale", "crops", "vit_heads", "swin_heads")}
    for f in ("plain.pth", "wrapped.pth"):
        got = EM.load_model(str(tmp_path / f), given)
        assert got["cfg"] == m["cfg"] and all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"])
    assert EM.DEFAULTS["taps"] == (6, 7, 8, 9) and EM.DEFAULTS["crops"] == 20 and EM.DEFAULTS["scale"] == 0.8
    bad = {k: v.numpy() for k, v in m["sd"].items()}
    del bad["tab2.1.k.bias"]
    np.savez(tmp_path / "missing.npz", **bad, **{"cfg.taps": np.asarray(m["cfg"]["taps"]), "cfg.vit_heads": np.asarray(2), "cfg.swin_heads": np.asarray(2)})
    with pytest.raises(EM.ManiqaError, match=r"missing\.npz: tab2\.1\.k\.bias missing"):
        EM.load_model(str(tmp_path / "missing.npz"))
    bad = {k: v.numpy() for k, v in m["sd"].items()}
    bad["swin1.1.0.attn.rpb"] = bad["swin1.1.0.attn.rpb"][:, :1]
    with pytest.raises(EM.ManiqaError, match=r"swin1\.1\.0\.attn\.rpb is \(49, 1\)"):
        EM.load_model(bad, given)
    assert maniqa.ManiqaError is EM.ManiqaError and issubclass(EM.ManiqaError, ValueError)


def test_the_pooled_score_is_over_all_crops_and_equal_crops_score_like_one():
    """65x65: every origin is 0, so the pooled score of 5 equal crops is the score of one."""
    m = MM.model("small")
    img = MM.image("65x65")
    five = EM.maniqa(img, m, None, torch.float64)
    one = EM.maniqa(img, m, [(0, 0)], torch.float64)
    sum_w = float(MM.reference("65x65")[2][1][0].sum())   # one crop's; the pooling eps 1e-8 weighs 5 times less against five crops' sum
    assert abs(five - one) <= 1.01 * one * (1e-8 / sum_w) * 0.8 + 1e-13 and abs(five - MM.reference("65x65")[0]) < 1e-15
    s, f, (ps, pw) = MM.reference("70x131")
    assert abs(s - float((pw * ps).sum() / (pw.sum() + 1e-8))) < 1e-15 and ps.shape == (5, 64)


# ---------------------------------------------------------------------------------------------------------------- command lines
def test_report_carries_maniqa_last(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    rep = Report(str(tmp_path / "r.csv"), lpips=True, niqe=True, clipiqa=True, musiq=True, maniqa=True)
    assert rep.header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq,maniqa"
    rep.add_scores("b.png", (30.0, 0.9, 0.1, 4.0, 0.5, 60.0, 0.25))
    rep.add("a.png", psnr=31.0, ssim=0.8, lpips=0.2, niqe=5.0, clipiqa=0.25, musiq=50.0, maniqa=0.75)
    assert rep.write()[-1] == "maniqa: 0.50000"
    assert read_report(str(tmp_path / "r.csv"))["a.png"] == (31.0, 0.8, 0.2, 5.0, 0.25, 50.0, 0.75)
    alone = Report(str(tmp_path / "a.csv"), maniqa=True, paired=False)
    assert alone.header() == "file,maniqa" and Report(None, maniqa=True).header() == "file,psnr_y,ssim_y,maniqa"
    nan = float("nan")
    assert alone.unscored((nan,)) == "maniqa" and alone.unscored((0.5,)) is None
    assert rep.unscored((30.0, 0.9, 0.1, 4.0, 0.5, nan, nan)) == "musiq"   # maniqa is looked at last
    with pytest.raises(MetricsError):
        Report(None, musiq=True).add("x", psnr=1.0, ssim=1.0, musiq=1.0, maniqa=0.5)
    with pytest.raises(MetricsError):
        alone.add("x")


def test_command_lines_parse_and_refuse_a_bad_model_file(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    for a in (inf.parse_args(), eval_batch.parse_args()):
        assert a.maniqa_model is None and a.maniqa_crops == "uniform" and a.maniqa_seed is None
    assert inf.load_maniqa_model(inf.parse_args()) is None
    missing = str(tmp_path / "nowhere.npz")
    monkeypatch.setattr(sys, "argv", base + ["--maniqa_model", missing])
    assert inf.parse_args().maniqa_model == missing and eval_batch.parse_args().maniqa_model == missing
    # refused before any model is touched: neither the device check nor the loaders run
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match="nowhere.npz"):
            main()
    m = MM.model("small")
    EM.save_npz(tmp_path / "good.npz", m)
    with np.load(tmp_path / "good.npz") as z:
        np.savez(tmp_path / "part.npz", **{k: z[k] for k in z.files if k != "weight.fc2.bias"})
    monkeypatch.setattr(sys, "argv", base + ["--maniqa_model", str(tmp_path / "part.npz")])
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match=r"part\.npz.*weight\.fc2\.bias missing"):
            main()
    assert touched == []
    assert "are not offered together with --shard_tiles, nor is --maniqa_model" in open(os.path.join(ROOT, "inference.py")).read()
    # --maniqa_crops random without a seed: the stated default
    monkeypatch.setattr(sys, "argv", base + ["--maniqa_model", str(tmp_path / "good.npz"), "--maniqa_crops", "random"])
    args = inf.parse_args()
    got = inf.load_maniqa_model(args)
    assert got["cfg"]["embed"] == 64 and got["cfg"]["crops"] == 5 and args.maniqa_crops == "random" and args.maniqa_seed == EM.DEFAULT_SEED == 231
    monkeypatch.setattr(sys, "argv", base + ["--maniqa_model", str(tmp_path / "good.npz"), "--maniqa_seed", "5"])
    with pytest.raises(SystemExit, match="--maniqa_seed"):   # a seed without random crops has no meaning
        inf.load_maniqa_model(inf.parse_args())
    monkeypatch.setattr(sys, "argv", ["evaluate_maniqa.py", "-i", "a", "--maniqa_model", "m.npz", "--backend", "gpu", "--ntest", "3", "--maniqa_crops", "random"])
    seen = {}
    monkeypatch.setattr(EM, "evaluate", lambda *a, **k: seen.update(k, args=a))
    EM.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "m.npz", 3) and seen["mode"] == "random" and seen["seed"] is None


def test_evaluate_maniqa_averages_a_folder(tmp_path):
    from PIL import Image
    EM.save_npz(tmp_path / "m.npz", MM.model("small"))
    for name in ("65x65", "70x131"):
        Image.fromarray(MM.image(name)).save(tmp_path / f"{name}.png")
    Image.fromarray(MM.ramp(64, 200, 1)).save(tmp_path / "short.png")
    lines = []
    avg = EM.evaluate(str(tmp_path), str(tmp_path / "m.npz"), log=lines.append)
    want = (MM.reference("65x65")[0] + MM.reference("70x131")[0]) / 2
    assert abs(avg - want) <= MM.gate()[0] and lines[-1] == f"maniqa: {avg:.5f}" and "1 not scored" in lines[-2]
