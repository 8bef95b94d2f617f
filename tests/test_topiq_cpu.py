"""tools/evaluate_topiq.py, the definition ir_topiq is tested against, and the host parts of the TOPIQ-NR scorer: no GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.support import topiq_model as TM

ET = TM.ET
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the gate
def test_gate_yardsticks():
    """fp32 against fp64 of the model on every case: this makes the gate."""
    ds, df = TM.pooled_host_deviation()
    gs, gf = TM.gate()
    for name in (c[0] for c in TM.CASES):
        hs, hf = TM.host_deviation(name)
        print(f"{name}: topiq_nr {TM.reference(name)[0]:.9f}; host fp32 deviation {hs:.3e} (score), " + ", ".join(f"{p} {v:.3e}" for p, v in zip(TM.PARTS, hf)))
    print(f"gate: {gs:.3e} (score), " + ", ".join(f"{p} {v:.3e}" for p, v in zip(TM.PARTS, gf)))
    assert 0 < ds and all(0 < v for v in df) and gs == TM.GATE_FACTOR * ds and gf == [TM.GATE_FACTOR * v for v in df] and TM.GATE_FACTOR == 8.0
    assert len(gf) == 6


def test_every_planted_bug_misses_the_gate_tenfold():
    gs, gf = TM.gate()
    assert set(TM.PLANTED_BUGS) == {"stride_on_conv1", "pool_floor_end", "pool_or", "chunk_swapped", "gelu_tanh", "bicubic_a05", "pos_halves_swapped",
                                    "memory_not_normed", "query_memory_swapped", "fine_to_coarse", "post_norm", "mean_before_pool"}
    for v in TM.PLANTED_BUGS:
        worst = 0.0
        for name in TM.SMALL:
            s, f, m = TM.run(name, torch.float64, v)
            ds, df = TM.deviations(s, f, m, name)
            worst = max(worst, ds / gs, max(d / g for d, g in zip(df, gf)))
        print(f"{v}: misses the gate {worst:.1f} times")
        assert worst > 10.0, v


def test_the_gates_of_the_seeded_models_are_alive():
    """The condition on the seeded weights, on the reference alone: the gate's sigmoid varies from pixel to pixel and is not saturated."""
    m = TM.model("small")
    x = ET.scaled_input(TM.image("64x64")).double()
    sd = m["sd"]
    f = F.relu(F.conv2d(x, sd["trunk.conv1.weight"].double(), None, 2, 3) * m["bn"]["trunk.bn1"][0].double()[None, :, None, None]
               + m["bn"]["trunk.bn1"][1].double()[None, :, None, None])
    x2 = F.conv2d(f, sd["gate.0.split.weight"].double(), sd["gate.0.split.bias"].double()).chunk(2, dim=1)[1]
    g = F.gelu(F.conv2d(x2, sd["gate.0.conv1.weight"].double(), sd["gate.0.conv1.bias"].double()))
    g = F.gelu(F.conv2d(g, sd["gate.0.conv2.weight"].double(), sd["gate.0.conv2.bias"].double(), 1, 1))
    g = torch.sigmoid(F.conv2d(g, sd["gate.0.conv3.weight"].double(), sd["gate.0.conv3.bias"].double(), 1, 1))
    print(f"gate 0 of 64x64: {float(g.min()):.3f} .. {float(g.max()):.3f}, std {float(g.std()):.3f}")
    assert 0.02 < float(g.min()) and float(g.max()) < 0.98 and float(g.std()) > 0.02


# ---------------------------------------------------------------------------------------------------------------- the model's parts
def test_sizes_and_the_pool_condition():
    assert ET.level_sizes(131, 97) == [(66, 49), (33, 25), (17, 13), (9, 7), (5, 4)]
    assert ET.token_sizes(131, 97) == [(5, 4)] * 5
    assert ET.level_sizes(16, 200) == [(8, 100), (4, 50), (2, 25), (1, 13), (1, 7)]
    assert ET.token_sizes(16, 200) == [(1, 7), (1, 7), (1, 7), (1, 13), (1, 7)]          # level 3 stays: its height is not above 1
    assert ET.token_sizes(16, 200, "pool_or")[3] == (1, 7)
    assert ET.level_sizes(33, 40)[4] == (2, 2) and ET.level_sizes(64, 64) == [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    assert ET.scorable(16, 16) and not ET.scorable(15, 100) and not ET.scorable(100, 15)
    with pytest.raises(ET.TopiqError, match="15 x 64"):
        ET.topiq(TM.ramp(15, 64, 1), TM.model("small"))


def test_adaptive_pool_is_torchs():
    g = torch.Generator().manual_seed(5)
    for H, W, th, tw in ((66, 49, 5, 4), (8, 100, 1, 7), (32, 32, 2, 2), (3, 5, 2, 2)):
        x = torch.randn((1, 3, H, W), generator=g, dtype=torch.float64)
        assert torch.allclose(ET.adaptive_pool(x, th, tw), F.adaptive_avg_pool2d(x, (th, tw)), rtol=0, atol=1e-14)
    x = torch.randn((1, 2, 66, 49), generator=g, dtype=torch.float64)
    assert not torch.allclose(ET.adaptive_pool(x, 5, 4, floor_end=True), F.adaptive_avg_pool2d(x, (5, 4)), atol=1e-3)


def test_position_table_is_torchs_bicubic_and_the_hosts_equals_the_models():
    from instarevive_amd import topiq
    m = TM.model("small")
    h_emb, w_emb = m["sd"]["h_emb"], m["sd"]["w_emb"]
    src = torch.cat([h_emb.double().expand(-1, -1, 32, 32), w_emb.double().expand(-1, -1, 32, 32)], dim=1)
    for H, W in ((5, 4), (1, 13), (1, 7), (2, 2), (32, 32), (40, 64)):
        tab = ET.position_table(h_emb, w_emb, H, W)
        want = F.interpolate(src, (H, W), mode="bicubic", align_corners=False)[0]
        assert tab.dtype == torch.float32 and tab.shape == (32, H, W)
        assert torch.allclose(tab.double(), want, rtol=0, atol=2e-7)                       # the written-out sum against torch's, both fp64, one rounding
        host = topiq.position_table(m, H, W)
        assert host.dtype == np.float32 and np.array_equal(host.view(np.uint32), tab.numpy().view(np.uint32))
    assert torch.equal(ET.position_table(h_emb, w_emb, 32, 32), src[0].float())             # at its own size the table is the embeddings
    assert not torch.allclose(ET.position_table(h_emb, w_emb, 5, 4, "bicubic_a05"), ET.position_table(h_emb, w_emb, 5, 4), atol=1e-4)


def test_attention_is_nn_multihead_attentions():
    m = TM.model("small")
    D, heads = 32, 2
    mha = torch.nn.MultiheadAttention(D, heads, batch_first=False).double()
    sd = m["sd"]
    mha.load_state_dict({"in_proj_weight": sd["ca.1.attn.in_proj_weight"].double(), "in_proj_bias": sd["ca.1.attn.in_proj_bias"].double(),
                         "out_proj.weight": sd["ca.1.attn.out_proj.weight"].double(), "out_proj.bias": sd["ca.1.attn.out_proj.bias"].double()})
    g = torch.Generator().manual_seed(9)
    q, kv = torch.randn((7, D), generator=g, dtype=torch.float64), torch.randn((13, D), generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = mha(q[:, None], kv[:, None], kv[:, None], need_weights=False)[0][:, 0]
        Wi, bi = sd["ca.1.attn.in_proj_weight"].double(), sd["ca.1.attn.in_proj_bias"].double()
        hd = D // heads
        qq = (F.linear(q, Wi[:D], bi[:D]) * hd ** -0.5).view(7, heads, hd).transpose(0, 1)
        kk = F.linear(kv, Wi[D:2 * D], bi[D:2 * D]).view(13, heads, hd).transpose(0, 1)
        vv = F.linear(kv, Wi[2 * D:], bi[2 * D:]).view(13, heads, hd).transpose(0, 1)
        got = F.linear((torch.softmax(qq @ kk.transpose(-1, -2), -1) @ vv).transpose(0, 1).reshape(7, D), sd["ca.1.attn.out_proj.weight"].double(),
                       sd["ca.1.attn.out_proj.bias"].double())
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_library_table_is_torchs_roundings():
    from instarevive_amd import topiq
    from instarevive_amd.build import build
    build()
    tab = topiq.input_table()
    assert tab.dtype == np.float32 and tab.shape == (3, 256) and np.array_equal(tab.view(np.uint32), ET.input_table().view(np.uint32))
    assert np.all(np.diff(tab, axis=1) > 0)


def test_header_symbols_and_build_list_move_together():
    from instarevive_amd import _lib
    from instarevive_amd.build import FILE_FLAGS, SOURCES
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    for s in ("ir_topiq_input_table", "ir_topiq_configure", "ir_topiq"):
        assert s in _lib.SYMBOLS and f"int {s}(" in header
    assert "IR_STAGE_TOPIQ = 28" in header and _lib.STAGE_TOPIQ == 28 and _lib.TOPIQ_NOT_CONFIGURED == -13
    assert "topiq.hip" in SOURCES and FILE_FLAGS["topiq.hip"] == ["-ffp-contract=off"]
    assert _lib.load_library().ir_abi_version() == 3   # exports are only added


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_loader_round_trips_an_npz_and_pyiqas_names(tmp_path):
    from instarevive_amd import topiq
    m = TM.model("small")
    ET.save_npz(tmp_path / "m.npz", m)
    got = topiq.load_model(str(tmp_path / "m.npz"))
    assert got["cfg"] == m["cfg"] and got["cfg"]["heads"] == 2 and set(got["sd"]) == set(m["sd"]) == set(ET.model_keys(m["cfg"]))
    assert all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"])
    pth = ET.to_pyiqa(m)
    assert set(ET.PYIQA_KEYS(m["cfg"]["depths"])) == set(m["sd"]) and len(pth) == len(m["sd"])
    assert "semantic_model.layer1.1.conv2.weight" in pth and "weight_pool.3.weight_blk.4.bias" in pth and "dim_reduce.0.0.weight" in pth
    assert "sa_attn_blks.2.layers.0.self_attn.in_proj_weight" in pth and "attn_blks.3.layers.0.multihead_attn.out_proj.bias" in pth
    assert "attn_blks.0.layers.0.norm3.weight" in pth and "attn_pool.self_attn.in_proj_bias" in pth and "score_linear.6.weight" in pth and "h_emb" in pth
    pth["semantic_model.bn1.num_batches_tracked"] = torch.tensor(7)
    torch.save(pth, tmp_path / "plain.pth")
    torch.save({"params": pth}, tmp_path / "wrapped.pth")
    for f in ("plain.pth", "wrapped.pth"):
        got = ET.load_model(str(tmp_path / f), 2)
        assert got["cfg"] == m["cfg"] and all(torch.equal(got["sd"][k], m["sd"][k]) for k in m["sd"])
    assert ET.load_model(str(tmp_path / "plain.pth"))["cfg"]["heads"] == ET.DEFAULT_HEADS == 4
    # a missing key, a surplus key, a wrong shape and a decoder self_attn key: each a TopiqError that names the key
    bad = {k: v for k, v in pth.items() if k != "attn_blks.2.layers.0.norm2.bias"}
    torch.save(bad, tmp_path / "missing.pth")
    with pytest.raises(ET.TopiqError, match=r"missing\.pth: ca\.2\.norm2\.bias missing"):
        ET.load_model(str(tmp_path / "missing.pth"))
    torch.save({**pth, "fc.weight": torch.zeros(3)}, tmp_path / "surplus.pth")
    with pytest.raises(ET.TopiqError, match=r"surplus\.pth: fc\.weight"):
        ET.load_model(str(tmp_path / "surplus.pth"))
    sd = dict(m["sd"])
    with pytest.raises(ET.TopiqError, match=r"extra\.thing"):
        ET.load_model({**sd, "extra.thing": torch.zeros(2)}, 2)
    sd["gate.3.conv2.weight"] = sd["gate.3.conv2.weight"][:, :, :, :1]
    with pytest.raises(ET.TopiqError, match=r"gate\.3\.conv2\.weight is \(64, 64, 3, 1\)"):
        ET.load_model(sd, 2)
    torch.save({**pth, "attn_blks.1.layers.0.self_attn.in_proj_weight": torch.zeros(96, 32)}, tmp_path / "selfattn.pth")
    with pytest.raises(ET.TopiqError, match=r"attn_blks\.1\.layers\.0\.self_attn\.in_proj_weight.*no self-attention"):
        ET.load_model(str(tmp_path / "selfattn.pth"))
    with pytest.raises(ET.TopiqError, match=r"ca\.1\.self_attn\.in_proj_weight"):
        ET.load_model({**m["sd"], "ca.1.self_attn.in_proj_weight": torch.zeros(96, 32)}, 2)
    assert topiq.TopiqError is ET.TopiqError and issubclass(ET.TopiqError, ValueError)


# ---------------------------------------------------------------------------------------------------------------- command lines
def test_report_column_orders_with_and_without_topiq(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    rep = Report(str(tmp_path / "r.csv"), lpips=True, niqe=True, clipiqa=True, musiq=True, maniqa=True, dists=True, topiq_nr=True)
    assert rep.header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq,maniqa,topiq_nr,dists"
    rep.add_scores("b.png", (30.0, 0.9, 0.1, 4.0, 0.5, 60.0, 0.25, 0.5, 0.3))
    rep.add("a.png", psnr=31.0, ssim=0.8, lpips=0.2, niqe=5.0, clipiqa=0.25, musiq=50.0, maniqa=0.75, topiq_nr=0.25, dists=0.1)
    lines = rep.write()
    assert lines[-2] == "topiq_nr: 0.37500" and lines[-1] == "dists: 0.20000"
    assert read_report(str(tmp_path / "r.csv"))["a.png"] == (31.0, 0.8, 0.2, 5.0, 0.25, 50.0, 0.75, 0.25, 0.1)
    alone = Report(str(tmp_path / "a.csv"), topiq_nr=True, paired=False)
    alone.add_scores("x.png", (0.5,))
    assert alone.header() == "file,topiq_nr" and alone.write() == ["topiq_nr: 0.50000"] and read_report(str(tmp_path / "a.csv")) == {"x.png": (0.5,)}
    assert Report(None, topiq_nr=True).header() == "file,psnr_y,ssim_y,topiq_nr"
    assert Report(None, musiq=True, topiq_nr=True, paired=False).header() == "file,musiq,topiq_nr"
    assert Report(None, ilniqe=True, topiq_nr=True, paired=False).header() == "file,ilniqe,topiq_nr"
    for h in (alone.header(), rep.header(), "file,psnr_y,ssim_y,topiq_nr", "file,musiq,topiq_nr", "file,maniqa,topiq_nr", "file,psnr_y,ssim_y,topiq_nr,dists"):
        assert h in Report.HEADERS_TOPIQ
    assert not any("topiq" in h for h in Report.HEADERS + Report.HEADERS_MANIQA + Report.HEADERS_DISTS)
    nan = float("nan")
    assert alone.unscored((nan,)) == "topiq_nr" and alone.unscored((0.5,)) is None
    assert rep.unscored((30.0, 0.9, 0.1, 4.0, 0.5, 60.0, nan, nan, nan)) == "maniqa"
    with pytest.raises(MetricsError):
        Report(None, musiq=True).add("x", psnr=1.0, ssim=1.0, musiq=1.0, topiq_nr=0.5)
    with pytest.raises(MetricsError):
        alone.add("x")
    # a report without the new column is byte-equal to today's
    old = Report(str(tmp_path / "old.csv"), lpips=True, niqe=True, clipiqa=True, musiq=True, maniqa=True, dists=True)
    old.add_scores("b.png", (30.0, 0.9, 0.1, 4.0, 0.5, 60.0, 0.25, 0.3))
    assert old.write() == ["psnr: 30.00000", "ssim: 0.90000", "lpips: 0.10000", "niqe: 4.00000", "clipiqa: 0.50000", "musiq: 60.00000", "maniqa: 0.25000", "dists: 0.30000"]
    assert (tmp_path / "old.csv").read_bytes() == b"file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq,maniqa,dists\nb.png,30.0,0.9,0.1,4.0,0.5,60.0,0.25,0.3\n"


def test_command_lines_parse_and_refuse_a_bad_model_file(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    for a in (inf.parse_args(), eval_batch.parse_args()):
        assert a.topiq_model is None
    assert inf.load_topiq_model(inf.parse_args()) is None
    missing = str(tmp_path / "nowhere.npz")
    monkeypatch.setattr(sys, "argv", base + ["--topiq_model", missing])
    assert inf.parse_args().topiq_model == missing and eval_batch.parse_args().topiq_model == missing
    # refused before any model is touched: neither the device check nor the loaders run
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    monkeypatch.setattr(inf, "load_niqe_params", lambda *a: touched.append("niqe"))
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match="nowhere.npz"):
            main()
    m = TM.model("small")
    ET.save_npz(tmp_path / "good.npz", m)
    with np.load(tmp_path / "good.npz") as z:
        np.savez(tmp_path / "part.npz", **{k: z[k] for k in z.files if k != "score.6.bias"})
    monkeypatch.setattr(sys, "argv", base + ["--topiq_model", str(tmp_path / "part.npz")])
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match=r"part\.npz.*score\.6\.bias missing"):
            main()
    assert touched == []
    monkeypatch.setattr(sys, "argv", base + ["--topiq_model", str(tmp_path / "good.npz"), "--shard_tiles"])
    with pytest.raises(SystemExit, match="--topiq_model is not offered together with --shard_tiles"):
        inf.load_topiq_model(inf.parse_args())
    monkeypatch.setattr(sys, "argv", base + ["--topiq_model", str(tmp_path / "good.npz")])
    got = inf.load_topiq_model(inf.parse_args())
    assert got["cfg"] == m["cfg"]
    monkeypatch.setattr(sys, "argv", ["evaluate_topiq.py", "-i", "a", "--topiq_model", "m.npz", "--backend", "gpu", "--ntest", "3"])
    seen = {}
    monkeypatch.setattr(ET, "evaluate", lambda *a, **k: seen.update(k, args=a))
    ET.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "m.npz", 3) and seen["heads"] is None


def test_evaluate_topiq_averages_a_folder(tmp_path):
    from PIL import Image
    ET.save_npz(tmp_path / "m.npz", TM.model("small"))
    for name in ("64x64", "33x40"):
        Image.fromarray(TM.image(name)).save(tmp_path / f"{name}.png")
    Image.fromarray(TM.ramp(12, 200, 1)).save(tmp_path / "short.png")
    lines = []
    avg, values = ET.evaluate(str(tmp_path), str(tmp_path / "m.npz"), log=lines.append)
    want = (TM.reference("64x64")[0] + TM.reference("33x40")[0]) / 2
    assert abs(avg - want) <= TM.gate()[0] and lines[-1] == f"topiq_nr: {avg:.5f}" and "1 not scored" in lines[-2] and sorted(values) == ["33x40.png", "64x64.png"]
