"""CLIP-IQA without a GPU: the gate of tests/test_clipiqa_gpu.py and the planted bugs that show what it tells apart, the library's input table,
BatchNorm folding, the loader's three file forms, tokenisation and the text side with a vocabulary built on the spot, the report's columns and the
command lines' flags."""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest
import torch

from tests.support import clipiqa_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EC = CM.EC
NAMES = [c[0] for c in CM.CASES]


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


# ---------------------------------------------------------------------------------------------------------------- the gate and what it tells apart
def test_gate_yardsticks_and_the_bf16_measurement():
    """The fp32 CPU model against the float64 model on every case: the yardsticks of the gate. No pair probability is saturated (reference()
    asserts 0.02 .. 0.98). bf16-rounded convolution operands miss the score gate on every case but the 1 x 1 one and the feature gate on every
    case: the reason the device path is exact fp32. Measured on one x86 host: fp32 score 4.3e-8 .. 4.5e-7, feature 4.1e-7 .. 4.5e-6; bf16 score
    3.1e-4 .. 1.1e-2, feature 4.4e-3 .. 1.0e-1."""
    gs, gf = CM.gate()
    for name in NAMES:
        hs, hf = CM.host_deviation(name)
        bs, bf = CM.bf16_deviation(name)
        print(f"{name}: score {CM.reference(name)[0]:.9f}; fp32 deviates {hs:.3e} / {hf:.3e} (score / feature), bf16 operands {bs:.3e} / {bf:.3e}")
        assert 0.0 < CM.reference(name)[0] < 1.0
        assert bf > gf
    print(f"gate: score {gs:.3e}, feature {gf:.3e}")
    # the gate is of the order of fp32 rounding through a deep network, far below the third decimal that is reported
    assert 1e-9 < gs < 1e-4 and 1e-8 < gf < 1e-3
    assert max(CM.bf16_deviation(n)[0] for n in NAMES) > 10 * gs


@pytest.mark.parametrize("bug", CM.PLANTED_BUGS)
def test_planted_bug_misses_the_gate_tenfold(bug):
    gs, gf = CM.gate()
    worst = 0.0
    for name in CM.SMALL:
        score, feat, _ = CM.run(name, variant=bug)
        ds, df = CM.deviations(score, feat, name)
        print(f"{bug} on {name}: score by {ds:.3e} ({ds / gs:.0f} x gate), feature by {df:.3e} ({df / gf:.0f} x gate)")
        worst = max(worst, ds / gs, df / gf)
    assert worst > 10.0


def test_batched_model_rows_equal_single_images():
    m = CM.model("small")
    imgs = [CM.ramp(70, 45, 5), CM.image("70x45")]
    scores, feats = EC.score_images(imgs, m, torch.float64)
    assert abs(scores[1] - CM.reference("70x45")[0]) < 1e-12 and np.allclose(feats[1], CM.reference("70x45")[1], rtol=0, atol=1e-10)
    assert EC.clipiqa(imgs[1], m, torch.float64) == pytest.approx(CM.reference("70x45")[0], abs=1e-12)
    for bad in (np.zeros((31, 64, 3), np.uint8), np.zeros((64, 64), np.uint8), np.zeros((64, 64, 3), np.float32)):
        with pytest.raises(EC.ClipIqaError):
            EC.clipiqa(bad, m)


# ---------------------------------------------------------------------------------------------------------------- the library's host parts
def test_library_table_is_torchs_roundings():
    from instarevive_amd import clipiqa
    tab = clipiqa.scaling_table()
    want = EC.scale_table()
    assert tab.shape == want.shape == (3, 256) and tab.dtype == want.dtype == np.float32
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32))      # all 768 entries, to the bit
    img = CM.image("70x45")
    assert np.array_equal(tab[np.arange(3)[:, None, None], img.transpose(2, 0, 1)], EC.scaled_input(img)[0].numpy())
    assert _library()[1].ir_clipiqa_scale_table(None) == -1


def test_header_symbols_and_build_list_move_together():
    L, lib = _library()
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "int ir_clipiqa(ir_ctx* ctx, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat_or_null," in header
    assert "int ir_clipiqa_configure(ir_ctx* ctx, const int layers[4], int width, int heads, int out_dim, int n_pairs, float logit_scale_exp);" in header
    assert "int ir_clipiqa_scale_table(float* tab768);" in header and "IR_STAGE_CLIPIQA = 15" in header
    assert {"ir_clipiqa", "ir_clipiqa_configure", "ir_clipiqa_scale_table"} <= set(L.SYMBOLS) and L.STAGE_CLIPIQA == 15
    assert all(hasattr(lib, n) for n in ("ir_clipiqa", "ir_clipiqa_configure", "ir_clipiqa_scale_table"))
    assert lib.ir_abi_version() == 3   # the entry points are additive
    from instarevive_amd import build
    assert "clipiqa.hip" in build.SOURCES
    flags = build.FLAGS + build.FILE_FLAGS.get("clipiqa.hip", [])
    assert [f for f in flags if f.startswith("-ffp-contract")][-1] == "-ffp-contract=off"
    # without a context: no workspace size, and the calls are refused
    assert lib.ir_workspace_bytes(None, L.STAGE_CLIPIQA, 1, 64, 64, 0, 0, 0) == 0
    assert lib.ir_clipiqa(None, None, None, 64, 192, 1, 64, 64, None, None, None, 0) == -1
    assert lib.ir_clipiqa_configure(None, (C.c_int * 4)(3, 4, 6, 3), 64, 32, 1024, 5, C.c_float(100.0)) == -1


def test_batchnorm_folds_to_one_scale_and_shift():
    """scale = g / sqrt(var + eps), shift = b - mean scale in float64 (what ir_clipiqa_configure computes before it rounds once) against the
    unfolded eval-mode BatchNorm in float64."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 5, 7, generator=g, dtype=torch.float64)
    w, var = torch.rand(64, generator=g, dtype=torch.float64) + 0.5, torch.rand(64, generator=g, dtype=torch.float64) + 0.5
    b, mean = torch.randn(64, generator=g, dtype=torch.float64) * 0.1, torch.randn(64, generator=g, dtype=torch.float64) * 0.1
    want = torch.nn.functional.batch_norm(x, mean, var, w, b, False, 0.0, EC.BN_EPS)
    scale = w / torch.sqrt(var + EC.BN_EPS)
    shift = b - mean * scale
    got = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    assert float((got - want).abs().max()) < 1e-14
    # rounded to fp32 once, the folded form stays within fp32 rounding of the unfolded one
    got32 = x.float() * scale.float().view(1, -1, 1, 1) + shift.float().view(1, -1, 1, 1)
    assert float((got32.double() - want).abs().max()) < 4e-6


# ---------------------------------------------------------------------------------------------------------------- loading
def _tiny():
    """A complete model of width 64 with one block per layer and an output of 64 values."""
    cfg = dict(layers=(1, 1, 1, 1), width=64, heads=32, out_dim=64)
    g = torch.Generator().manual_seed(5)
    sd = {k: (torch.rand(s, generator=g) + 0.5 if k.endswith("running_var") else torch.randn(s, generator=g) * 0.05) for k, s in EC.visual_keys(cfg).items()}
    sd["visual.bn1.num_batches_tracked"] = torch.tensor(7)
    sd["visual.attnpool.positional_embedding"] = torch.randn(50, 2048, generator=g)
    sd["logit_scale"] = torch.tensor(float(np.log(100.0)))
    return sd, cfg


def _vocabulary(folder):
    """A BPE table built on the spot from the prompts' own words, written as open_clip's file; the tokenizer over it."""
    from instarevive_amd.clip_bpe import ClipBPETokenizer
    words = sorted({w for p in EC.PROMPTS for w in p.lower().replace("-", " - ").split()})
    merges = []
    for w in words:   # merge every word left to right into one token
        parts = list(w[:-1]) + [w[-1] + "</w>"]
        while len(parts) > 1:
            if (parts[0], parts[1]) not in merges:
                merges.append((parts[0], parts[1]))
            parts = [parts[0] + parts[1]] + parts[2:]
    os.makedirs(folder, exist_ok=True)
    with gzip.open(os.path.join(folder, "bpe_simple_vocab_16e6.txt.gz"), "wt", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(" ".join(m) for m in merges) + "\n")
    return ClipBPETokenizer.from_folder(str(folder))


def _text_tower(vocab, width=64, layers=2, context=12, out_dim=64, seed=9):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * 0.2
    sd = {"token_embedding.weight": r(vocab, width), "positional_embedding": r(context, width), "ln_final.weight": 1 + r(width), "ln_final.bias": r(width),
          "text_projection": r(width, out_dim)}
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        sd.update({p + "ln_1.weight": 1 + r(width), p + "ln_1.bias": r(width), p + "ln_2.weight": 1 + r(width), p + "ln_2.bias": r(width),
                   p + "attn.in_proj_weight": r(3 * width, width), p + "attn.in_proj_bias": r(3 * width), p + "attn.out_proj.weight": r(width, width),
                   p + "attn.out_proj.bias": r(width), p + "mlp.c_fc.weight": r(4 * width, width), p + "mlp.c_fc.bias": r(4 * width),
                   p + "mlp.c_proj.weight": r(width, 4 * width), p + "mlp.c_proj.bias": r(width)})
    return sd


def test_prompts_tokenise_and_the_text_side_matches_torchs_own_modules(tmp_path):
    """The ten prompts through clip_bpe over a vocabulary built on the spot (one token per word; start, words, end, zero padding), and
    encode_text against the same tower assembled from torch.nn modules (MultiheadAttention with a causal mask, LayerNorm, QuickGELU)."""
    tok = _vocabulary(tmp_path / "bpe")
    rows = tok(list(EC.PROMPTS), 12)
    assert rows.shape == (10, 12) and bool((rows[:, 0] == tok.sot).all())
    for row, p in zip(rows, EC.PROMPTS):
        words = p.lower().replace("-", " - ").split()
        assert int(row[1 + len(words)]) == tok.eot and bool((row[2 + len(words):] == 0).all()) and int(row.argmax()) == 1 + len(words)
        assert [int(v) for v in row[1:1 + len(words)]] == [tok.encoder[w + "</w>"] for w in words]
    assert rows[0].tolist() != rows[1].tolist()
    sd = _text_tower(len(tok.encoder))
    got = EC.encode_text(sd, rows)
    width = 64
    x = torch.nn.functional.embedding(rows, sd["token_embedding.weight"]) + sd["positional_embedding"]
    mask = torch.full((12, 12), float("-inf")).triu(1)
    for i in range(2):
        p = f"transformer.resblocks.{i}."
        attn = torch.nn.MultiheadAttention(width, 1, batch_first=True)
        attn.load_state_dict({"in_proj_weight": sd[p + "attn.in_proj_weight"], "in_proj_bias": sd[p + "attn.in_proj_bias"],
                              "out_proj.weight": sd[p + "attn.out_proj.weight"], "out_proj.bias": sd[p + "attn.out_proj.bias"]})
        h = torch.nn.functional.layer_norm(x, (width,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"])
        x = x + attn(h, h, h, need_weights=False, attn_mask=mask)[0].detach()
        h = torch.nn.functional.layer_norm(x, (width,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"])
        h = torch.nn.functional.linear(h, sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"])
        x = x + torch.nn.functional.linear(h * torch.sigmoid(1.702 * h), sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"])
    x = torch.nn.functional.layer_norm(x, (width,), sd["ln_final.weight"], sd["ln_final.bias"])
    want = x[torch.arange(10), rows.argmax(-1)] @ sd["text_projection"]
    assert got.shape == (10, 64) and float((got - want).abs().max()) < 1e-5 * float(want.abs().max())
    text = EC.text_features(sd, tok)
    assert torch.allclose(text.norm(dim=1), torch.ones(10), atol=1e-6) and torch.allclose(text, torch.nn.functional.normalize(want, dim=1), atol=1e-5)


def test_loader_reads_a_state_dict_an_npz_and_a_torchscript_archive(tmp_path):
    from instarevive_amd import clipiqa
    tok = _vocabulary(tmp_path / "bpe")
    sd, cfg = _tiny()
    sd.update(_text_tower(len(tok.encoder)))
    # a plain state dict, in half precision as OpenAI's file is: upcast, shape read off the tensors
    torch.save({k: (v.half() if v.is_floating_point() else v) for k, v in sd.items()}, tmp_path / "m.pt")
    a = clipiqa.load_model(str(tmp_path / "m.pt"), str(tmp_path / "bpe"))
    assert a["cfg"] == cfg and a["text"].shape == (10, 64) and a["text"].dtype == torch.float32 and abs(a["logit_scale_exp"] - 100.0) < 0.1
    assert all(v.dtype == torch.float32 for v in a["sd"].values()) and torch.equal(a["sd"]["visual.conv1.weight"], sd["visual.conv1.weight"].half().float())
    # an .npz with the same names; with `text` no vocabulary is needed
    np.savez(tmp_path / "m.npz", **{k: v.numpy() for k, v in sd.items()})
    b = clipiqa.load_model(str(tmp_path / "m.npz"), str(tmp_path / "bpe"))
    assert b["cfg"] == cfg and torch.equal(b["sd"]["visual.conv1.weight"], sd["visual.conv1.weight"])
    assert torch.allclose(a["text"], b["text"], atol=2e-2)                 # a's weights went through fp16
    np.savez(tmp_path / "t.npz", text=b["text"].numpy() * 3.0, **{k: v.numpy() for k, v in sd.items() if k.startswith("visual.") or k == "logit_scale"})
    c = clipiqa.load_model(str(tmp_path / "t.npz"))
    assert torch.allclose(c["text"], b["text"], atol=1e-6)                 # rows are normalised on the way in
    # a TorchScript archive made on the spot from a module that holds the same names
    class Holder(torch.nn.Module):
        def forward(self, x):
            return x

    def plant(root, name, value, buffer):
        parts = name.split(".")
        for p in parts[:-1]:
            if not hasattr(root, p):
                root.add_module(p, Holder())
            root = getattr(root, p)
        root.register_buffer(parts[-1], value) if buffer else root.register_parameter(parts[-1], torch.nn.Parameter(value, requires_grad=False))

    holder = Holder()
    for k, v in sd.items():
        plant(holder, k, v, not v.is_floating_point() or "running" in k)
    torch.jit.script(holder).save(str(tmp_path / "m.jit.pt"))
    d = clipiqa.load_model(str(tmp_path / "m.jit.pt"), str(tmp_path / "bpe"))
    assert d["cfg"] == cfg and torch.equal(d["text"], b["text"]) and all(torch.equal(d["sd"][k], b["sd"][k]) for k in b["sd"])
    # the same image scores alike through every form
    img = CM.image("32x32")
    assert EC.clipiqa(img, b) == EC.clipiqa(img, d) and abs(EC.clipiqa(img, a) - EC.clipiqa(img, b)) < 0.05
    # refusals name the file and the tensor
    np.savez(tmp_path / "short.npz", **{k: v.numpy() for k, v in sd.items() if k != "visual.layer3.0.bn2.running_mean"})
    with pytest.raises(EC.ClipIqaError, match=r"short\.npz.*visual\.layer3\.0\.bn2\.running_mean"):
        clipiqa.load_model(str(tmp_path / "short.npz"), str(tmp_path / "bpe"))
    np.savez(tmp_path / "shape.npz", **{k: (v.numpy()[:-1] if k == "visual.attnpool.c_proj.bias" else v.numpy()) for k, v in sd.items()})
    with pytest.raises(EC.ClipIqaError, match=r"shape\.npz.*visual\.attnpool\.c_proj\.bias"):
        clipiqa.load_model(str(tmp_path / "shape.npz"), str(tmp_path / "bpe"))
    with pytest.raises(EC.ClipIqaError, match="BPE"):
        clipiqa.load_model(str(tmp_path / "m.npz"))
    assert clipiqa.ClipIqaError is EC.ClipIqaError


# ---------------------------------------------------------------------------------------------------------------- report and command lines
def test_report_columns_for_every_flag_combination(tmp_path):
    from instarevive_amd.metrics import MetricsError, Report, read_report
    values = dict(psnr=30.5, ssim=0.9, lpips=0.25, niqe=6.5, clipiqa=0.625)
    for paired in (True, False):
        for lp in (False, True):
            for nq in (False, True):
                for cq in (False, True):
                    if not paired and (lp or not (nq or cq)):
                        with pytest.raises(MetricsError):
                            Report(None, lpips=lp, niqe=nq, paired=paired, clipiqa=cq)
                        continue
                    keys = (("psnr", "ssim") if paired else ()) + (("lpips",) if lp else ()) + (("niqe",) if nq else ()) + (("clipiqa",) if cq else ())
                    path = tmp_path / f"r{paired:d}{lp:d}{nq:d}{cq:d}.csv"
                    rep = Report(str(path), lpips=lp, niqe=nq, paired=paired, clipiqa=cq)
                    rep.add_scores("b.png", tuple(values[k] for k in keys))
                    rep.add("a.png", **{k: values[k] + 1 for k in keys})
                    assert rep.write() == [f"{k}: {values[k] + 0.5:.5f}" for k in keys]
                    header = ",".join(("file",) + tuple({"psnr": "psnr_y", "ssim": "ssim_y"}.get(k, k) for k in keys))
                    assert path.read_text().splitlines()[0] == header and header in Report.HEADERS
                    assert "file,psnr_y,ssim_y,lpips,niqe,clipiqa".startswith(header) or not (paired and lp and nq)
                    assert read_report(str(path)) == {"b.png": tuple(values[k] for k in keys), "a.png": tuple(values[k] + 1 for k in keys)}
                    with pytest.raises(MetricsError):
                        rep.add_scores("x", tuple(values[k] for k in keys) + (1.0,))
                    if not cq:
                        with pytest.raises(MetricsError):
                            rep.add("x", **{k: values[k] for k in keys}, clipiqa=0.5)
    full = Report(None, lpips=True, niqe=True, clipiqa=True)
    assert full.header() == "file,psnr_y,ssim_y,lpips,niqe,clipiqa"
    assert Report(None, clipiqa=True, paired=False).header() == "file,clipiqa"


def test_command_lines_parse_and_refuse_a_bad_model_file(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"]
    monkeypatch.setattr(sys, "argv", base)
    assert inf.parse_args().clipiqa_model is None and eval_batch.parse_args().clipiqa_model is None and inf.parse_args().clip_bpe is None
    assert inf.load_clipiqa_model(inf.parse_args()) is None
    missing = str(tmp_path / "nowhere.pt")
    monkeypatch.setattr(sys, "argv", base + ["--clipiqa_model", missing, "--clip_bpe", "v"])
    assert inf.parse_args().clipiqa_model == missing and eval_batch.parse_args().clipiqa_model == missing and eval_batch.parse_args().clip_bpe == "v"
    # refused before any model is touched: neither the device check nor the loaders run
    touched = []
    monkeypatch.setattr(inf, "check_device", lambda d: touched.append("device") or d)
    monkeypatch.setattr(inf, "load_models", lambda *a: touched.append("models"))
    for main in (inf.main, eval_batch.main):
        with pytest.raises(SystemExit, match="nowhere.pt"):
            main()
    sd, _ = _tiny()
    np.savez(tmp_path / "notext.npz", **{k: v.numpy() for k, v in sd.items()})
    monkeypatch.setattr(sys, "argv", base + ["--clipiqa_model", str(tmp_path / "notext.npz")])
    with pytest.raises(SystemExit, match=r"notext\.npz.*BPE"):
        inf.main()
    monkeypatch.setattr(sys, "argv", base + ["--clip_bpe", "v"])
    with pytest.raises(SystemExit, match="--clip_bpe needs --clipiqa_model"):
        inf.main()
    assert touched == []
    text = torch.nn.functional.normalize(torch.randn(10, 64, generator=torch.Generator().manual_seed(1)), dim=1)
    np.savez(tmp_path / "good.npz", text=text.numpy(), **{k: v.numpy() for k, v in sd.items()})
    monkeypatch.setattr(sys, "argv", base + ["--clipiqa_model", str(tmp_path / "good.npz")])
    got = inf.load_clipiqa_model(inf.parse_args())
    assert got["cfg"]["layers"] == (1, 1, 1, 1) and torch.allclose(got["text"], text, atol=1e-6)
    monkeypatch.setattr(sys, "argv", ["evaluate_clipiqa.py", "-i", "a", "--clipiqa_model", "m.npz", "--clip_bpe", "v", "--backend", "gpu", "--ntest", "3"])
    seen = {}
    monkeypatch.setattr(EC, "evaluate", lambda *a, **k: seen.update(k, args=a))
    EC.main()
    assert seen["backend"] == "gpu" and seen["args"] == ("a", "m.npz", "v", 3)


def test_evaluate_clipiqa_averages_a_folder(tmp_path):
    from PIL import Image
    m = CM.model("small")
    np.savez(tmp_path / "m.npz", text=m["text"].numpy(), **{k: v.numpy() for k, v in m["sd"].items()})
    for name in ("32x32", "70x45"):
        Image.fromarray(CM.image(name)).save(tmp_path / f"{name}.png")
    Image.fromarray(CM.ramp(20, 64, 1)).save(tmp_path / "small.png")
    lines = []
    avg = EC.evaluate(str(tmp_path), str(tmp_path / "m.npz"), log=lines.append)
    want = (CM.reference("32x32")[0] + CM.reference("70x45")[0]) / 2
    assert abs(avg - want) <= CM.gate()[0] and lines[-1] == f"clipiqa: {avg:.5f}" and "1 not scored" in lines[-2]
