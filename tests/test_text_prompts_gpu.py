"""Prompts as text on the GPU: the stream-ordered T5 encode against ir_t5_encode, the caption cache's fp16 store and its gather bit for bit, the
command lines' text routes against their file routes byte for byte, and the device's answer to ids outside the vocabulary.

Models are seeded and small, as in tests/test_cli_gpu.py: a SentencePiece model trained on the spot and a 2-layer T5 v1.1 encoder whose d_model is the
small DiT's caption width (64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests.golden._det import det_input, det_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(d_model=64, d_kv=16, num_heads=4, d_ff=128, num_layers=2)
CAPTIONS = ["a high quality photo of a human face", "a photo of a cat and a dog in the garden", "", "clean, realistic, natural skin texture, sharp focus, 8k " * 4]


@pytest.fixture(scope="module")
def t5_dir(tmp_path_factory):
    """A folder in the DeepFloyd layout: spiece.model, config.json, model.safetensors."""
    import sentencepiece as spm
    from safetensors.torch import save_file
    from transformers import T5Tokenizer
    from oracle import t5 as ot5
    d = tmp_path_factory.mktemp("t5")
    corpus = d / "corpus.txt"
    corpus.write_text("\n".join(["a high quality photo of a human face", "highly detailed portrait, sharp focus, 8k", "restore the image cleanly",
                                 "a photo of a cat and a dog in the garden", "clean, realistic, natural skin texture"] * 4))
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(d / "spiece"), vocab_size=60, model_type="unigram", pad_id=0, eos_id=1, unk_id=2,
                                   bos_id=-1, hard_vocab_limit=False, minloglevel=2)
    os.remove(corpus)
    tok = T5Tokenizer.from_pretrained(str(d))
    cfg = dict(CFG, vocab_size=len(tok))
    sd = det_state_dict(ot5.state_dict_shapes(cfg), seed=717)
    sd["shared.weight"] = sd["shared.weight"] * 8.0
    for k in sd:
        if k.endswith("SelfAttention.q.weight"):
            sd[k] = sd[k] * cfg["d_kv"] ** -0.5
    (d / "config.json").write_text(json.dumps(dict(cfg, feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6, relative_attention_num_buckets=32,
                                                   relative_attention_max_distance=128, model_type="t5")))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    return d


@pytest.fixture(scope="module")
def t5(t5_dir):
    from instarevive_amd import text_prompts as TP
    return TP.load_tokenizer(t5=str(t5_dir)), TP.load_encoder("cuda", t5=str(t5_dir))


@pytest.fixture(scope="module")
def artifacts(tmp_path_factory):
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path_factory.mktemp("models")
    _write_artifacts(d)
    return d


def _model_flags(d):
    return ["--ckpt", str(d / "weights" / "dit.ckpt"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"),
            "--vae", str(d / "vae"), "--dit_config", str(d / "pixart")]


def _run(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + flags, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _files(folder):
    out = {}
    for root, _, names in os.walk(folder):
        for nm in names:
            if nm.endswith(".png"):
                with open(os.path.join(root, nm), "rb") as f:
                    out[os.path.relpath(os.path.join(root, nm), folder)] = f.read()
    return out


# ------------------------------------------------------------------------------------------------ 1. encode parity
@pytest.mark.parametrize("tokens", [24, 72])   # below ir_dit_set_prompts' 64-token bucket and not a multiple of it; across it
def test_stream_ordered_encode_equals_ir_t5_encode_bit_for_bit(t5, tokens):
    from instarevive_amd.text_prompts import tokenize
    tok, enc = t5
    for b in (1, 3):
        texts = ["", CAPTIONS[3], CAPTIONS[0]][:b]   # b = 1: a prompt that is only EOS + padding; b = 3 adds a truncated and a short one
        ids, mask = tokenize(tok, texts, tokens)
        assert int(mask[0].sum()) == 1
        want = enc(input_ids=ids, attention_mask=mask)["last_hidden_state"]
        enc.prepare(b, tokens)
        di, dm = ids.to("cuda", torch.int32), mask.to("cuda", torch.float32)
        got = enc.encode_prompts(di, dm, torch.full((b, tokens, CFG["d_model"]), float("nan"), device="cuda"))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(torch.isfinite(got).all()), (tokens, b)
    assert enc.status() == 0


def test_encode_refuses_a_length_whose_bias_table_was_not_uploaded(t5):
    """Nothing is uploaded on first use: the table belongs to the prompt source's set-up."""
    tok, enc = t5
    ids = torch.ones(1, 31, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="t5.bias table"):
        enc.encode_prompts(ids, torch.ones(1, 31, device="cuda"), torch.empty(1, 31, CFG["d_model"], device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. the cache store
def _store(ctx, x, mask, cache, cache_mask, slot0):
    from instarevive_amd import _lib as L
    fp16 = cache.dtype == torch.float16
    ctx.check(ctx.lib.ir_prompt_cache_store(ctx.h, ctx.stream(), L.ptr(x), L.ptr(mask), L.ptr(cache), L.ptr(cache_mask), int(fp16), cache.shape[0], slot0,
                                            x.shape[0], x.shape[1], x.shape[2]), "ir_prompt_cache_store")


def _rounding_cases():
    """fp32 values at fp16 rounding ties (both parities of the kept bit), around the subnormal limit 2^-14 and the smallest subnormal 2^-24 (2^-25 is
    the tie to zero), around the largest finite 65504 (65520 is the tie to infinity), their negatives, zeros and values far outside."""
    e = lambda k: 2.0 ** k
    v = [1 + e(-11), 1 + 3 * e(-11), 1 + e(-11) + e(-23), 1 + e(-11) - e(-24), 1 + e(-10), 2047.5, 2048.5, 2049.0, 2051.0, 0.1, 1 / 3,
         e(-14), e(-14) - e(-25), e(-14) * (1 - e(-12)), e(-15), 3 * e(-25), e(-24), e(-24) + e(-26), 1.5 * e(-24), 2.5 * e(-24), e(-25), e(-25) * (1 + e(-23)),
         e(-25) * (1 - e(-24)), e(-26), 1e-10, 1e-30, 1e-40, 0.0,
         65504.0, 65504.0 + 8, 65519.996, 65520.0, 65520.004, 65536.0, 70000.0, 1e10, 3e38, float("inf")]
    return torch.tensor(v + [-a for a in v], dtype=torch.float64).to(torch.float32)


def test_cache_store_rounds_to_fp16_as_torch_does_bit_for_bit(ctx):
    cases = _rounding_cases()
    g = torch.Generator().manual_seed(5)
    # [2][7][64]: one block, the cases first; [3][301][68]: 57 blocks of a grid-stride loop, a width that is no multiple of 64, values over 40 binades
    for shape, slot0, slots in (((2, 7, 64), 1, 4), ((3, 301, 68), 0, 3)):
        x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-30, 18, shape, generator=g).float())
        x.view(-1)[:cases.numel()] = cases
        mask = (torch.rand(shape[:2], generator=g) < 0.5).float()
        want = x.to(torch.float16)
        xd = x.cuda()
        assert torch.equal(xd.to(torch.float16).cpu().view(torch.int16), want.view(torch.int16))
        for dtype in (torch.float16, torch.float32):
            cache = torch.full((slots,) + shape[1:], 3.0, dtype=dtype, device="cuda")
            cmask = torch.full((slots, shape[1]), 3.0, device="cuda")
            _store(ctx, xd, mask.cuda(), cache, cmask, slot0)
            got = cache[slot0:slot0 + shape[0]].cpu()
            if dtype == torch.float16:
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), shape
                k = cases.numel()
                assert torch.isinf(got.view(-1)[:k]).sum() == torch.isinf(want.view(-1)[:k]).sum() >= 10 and (got.view(-1)[:k] == 0).sum() >= 10
            else:
                assert torch.equal(got.view(torch.int32), x.view(torch.int32))
            assert torch.equal(cmask[slot0:slot0 + shape[0]].cpu(), mask)
            rest = torch.cat([cache[:slot0], cache[slot0 + shape[0]:]]).float()
            assert bool((rest == 3.0).all()) and bool((torch.cat([cmask[:slot0], cmask[slot0 + shape[0]:]]) == 3.0).all())   # the other slots are untouched
    # a store that would leave the cache is refused on the host
    from instarevive_amd import _lib as L
    cache = torch.zeros(2, 7, 64, dtype=torch.float16, device="cuda")
    x = torch.zeros(2, 7, 64, device="cuda")
    assert ctx.lib.ir_prompt_cache_store(ctx.h, ctx.stream(), L.ptr(x), None, L.ptr(cache), L.ptr(torch.zeros(2, 7, device="cuda")), 1, 2, 1, 2, 7, 64) == -10


# ------------------------------------------------------------------------------------------------ 3. the gather
def _gather(ctx, cache, cmask, slots, fixed, fmask):
    from instarevive_amd import _lib as L
    n, (T, D) = len(slots), fixed.shape
    y, bias = torch.full((n, T, D), float("nan"), device="cuda"), torch.full((n, T), float("nan"), device="cuda")
    ds = torch.tensor(slots, dtype=torch.int32, device="cuda")
    ctx.check(ctx.lib.ir_prompt_gather(ctx.h, ctx.stream(), L.ptr(cache), L.ptr(cmask), int(cache.dtype == torch.float16), cache.shape[0], L.ptr(ds), L.ptr(fixed),
                                       L.ptr(fmask), L.ptr(y), L.ptr(bias), n, T, D), "ir_prompt_gather")
    return y.cpu(), bias.cpu()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_gather_equals_a_host_built_block_bit_for_bit(ctx, dtype):
    T, D = 301, 68   # several blocks per image, no multiple of anything
    cache = det_input(31, (3, T, D), -4, 4).to(dtype)
    cmask = (det_input(32, (3, T)) < 0.6).float()
    fixed, fmask = det_input(33, (T, D), -4, 4), (det_input(34, (T,)) < 0.3).float()
    dev = [t.cuda() for t in (cache, cmask, fixed, fmask)]
    y, bias = _gather(ctx, *dev[:2], [2, -1, 0], *dev[2:])
    want = torch.stack([cache[2].float(), fixed, cache[0].float()])
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert torch.equal(bias, torch.stack([cmask[2], fmask, cmask[0]])) and set(bias.unique().tolist()) == {0.0, 1.0}   # the mask's values as they are
    y1, b1 = _gather(ctx, *dev[:2], [-1], *dev[2:])
    assert torch.equal(y1[0].view(torch.int32), fixed.view(torch.int32)) and torch.equal(b1[0], fmask)


# ------------------------------------------------------------------------------------------------ 4. the text route equals the file route
def _inputs(folder, sizes, seed):
    os.makedirs(folder / "sub", exist_ok=True)
    names = ["a.png", "sub/b.png", "c.png", "d.png"][:len(sizes)]
    for i, (nm, hw) in enumerate(zip(names, sizes)):
        Image.fromarray((det_input(seed + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(folder / nm)
    return names


def test_inference_captions_equals_caption_dir_byte_for_byte(tmp_path, artifacts, t5_dir):
    d = tmp_path
    _inputs(d / "in", [(64, 64), (40, 56), (64, 64)], 500)
    (d / "caps.json").write_text(json.dumps({"a.png": CAPTIONS[0], "sub/b.png": CAPTIONS[1]}))   # c.png has no caption: the fixed prompt
    base = _model_flags(artifacts) + ["--input", str(d / "in"), "--prompt_embeds", str(artifacts / "prompt.pth")]
    out = _run("inference.py", base + ["--output", str(d / "text"), "--captions", str(d / "caps.json"), "--save_captions", str(d / "npz"), "--t5", str(t5_dir)])
    assert "2 captions were T5-encoded" in out and "GB of weights" in out
    with np.load(d / "npz" / "sub" / "b.npz") as z:
        assert z["caption_feature"].dtype == np.float16 and z["caption_feature"].shape == (1, 20, 64) and z["attention_mask"].dtype == np.int16
        assert z["attention_mask"].shape == (1, 20) and 2 < int(z["attention_mask"].sum()) <= 20
    assert sorted(os.listdir(d / "npz")) == ["a.npz", "sub"]
    _run("inference.py", base + ["--output", str(d / "file"), "--caption_dir", str(d / "npz")])
    text, file = _files(d / "text"), _files(d / "file")
    assert sorted(text) == sorted(file) == ["a_0.png", "c_0.png", "sub/b_0.png"]
    for k in text:
        assert text[k] == file[k], k


def test_eval_batch_captions_equals_caption_dir_at_batch_size_3(tmp_path, artifacts, t5_dir):
    d = tmp_path
    _inputs(d / "in", [(70, 90), (64, 64), (97, 71), (64, 100)], 520)
    caps = d / "caps"
    os.makedirs(caps / "sub")
    (caps / "a.txt").write_text(CAPTIONS[0] + "\n")
    (caps / "sub" / "b.txt").write_text(CAPTIONS[1])
    (caps / "d.txt").write_text(CAPTIONS[0])           # a repeated caption: encoded once (c.png has none: the fixed prompt inside a batch of 3)
    base = _model_flags(artifacts) + ["--input", str(d / "in"), "--prompt_embeds", str(artifacts / "prompt.pth"), "--batch_size", "3", "--image_size", "64"]
    out = _run("eval_batch.py", base + ["--output", str(d / "text"), "--captions", str(caps), "--save_captions", str(d / "npz"), "--t5", str(t5_dir)])
    assert "2 captions were T5-encoded in the run, 3 caption files written" in out
    _run("eval_batch.py", base + ["--output", str(d / "file"), "--caption_dir", str(d / "npz")])
    for sub in ("text", "text-cond"):
        a, b = _files(d / sub), _files(d / sub.replace("text", "file"))
        assert sorted(a) == sorted(b) and len(a) == 4
        for k in a:
            assert a[k] == b[k], (sub, k)


def test_make_captions_writes_the_reference_caption_files(tmp_path, t5_dir, t5):
    """tools/make_captions.py under extract_caption.py's flags: one npz per JSON key, the bits of an encode and fp16 store made here."""
    from instarevive_amd import prompts
    from instarevive_amd import text_prompts as TP
    table = {"a.png": CAPTIONS[0], "sub/b.jpg": "  " + CAPTIONS[1] + " \n", "c.png": ""}
    (tmp_path / "caps.json").write_text(json.dumps(table))
    out = _run(os.path.join("tools", "make_captions.py"), ["--t5_json_path", str(tmp_path / "caps.json"), "--t5_models_dir", str(t5_dir), "--t5_save_root",
                                                          str(tmp_path / "npz"), "--max_length", "20", "--batch_size", "1"])
    assert "saved 3 caption files" in out
    tok, enc = t5
    be = TP.DeviceBackend(enc, 20, 1, 1)
    for key, cap in table.items():
        be.encode_store(*TP.tokenize(tok, [cap.strip()], 20), [0])
        want_y, want_m = be.read_slot(0)
        path = str(tmp_path / "npz" / (os.path.splitext(key)[0] + ".npz"))
        with np.load(path) as z:
            assert z["caption_feature"].dtype == np.float16 and z["caption_feature"].shape == (1, 20, 64) and z["attention_mask"].dtype == np.int16
            assert np.array_equal(z["caption_feature"][0].view(np.int16), want_y.numpy().view(np.int16)) and np.array_equal(z["attention_mask"][0], want_m.numpy())
        y, m = prompts.load_caption(path)
        assert torch.equal(y, want_y.float()) and torch.equal(m, want_m) and int(m.sum()) == (1 if cap == "" else int(m.sum())) >= 1


# ------------------------------------------------------------------------------------------------ 5. the fixed prompt route
def test_prompt_flag_equals_prompt_embeds_over_make_prompts_file(tmp_path, artifacts, t5_dir, t5):
    from tools.make_prompt import make_prompt
    d = tmp_path
    _inputs(d / "in", [(64, 64), (40, 56)], 540)
    text = "A high quality PHOTO of a human face, <b>highly detailed</b>"
    tok, enc = t5
    torch.save(make_prompt(tok, enc, text, 24, clean=True), d / "typed.pth")    # what tools/make_prompt.py --prompt X --max_length 24 --clean writes
    base = _model_flags(artifacts) + ["--input", str(d / "in")]
    out = _run("inference.py", base + ["--output", str(d / "text"), "--prompt", text, "--clean_captions", "--prompt_max_length", "24", "--t5", str(t5_dir)])
    assert "the encoder's memory is released" in out
    _run("inference.py", base + ["--output", str(d / "file"), "--prompt_embeds", str(d / "typed.pth")])
    a, b = _files(d / "text"), _files(d / "file")
    assert sorted(a) == sorted(b) and len(a) == 2
    for k in a:
        assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ 6. the prompt reaches the network
def test_a_caption_changes_its_own_image_and_no_other_of_the_batch(tmp_path, t5):
    from instarevive_amd import text_prompts as TP
    from instarevive_amd.pipeline import process_stream
    from tests import test_models_gpu as M
    tok, enc = t5
    (sw, _), (vae, _), (dit, _) = M._small_models()
    y, mask3 = M._prompt(M.DIT_SMALL)
    names = _inputs(tmp_path / "in", [(64, 64)] * 3, 560)
    paths = [str(tmp_path / "in" / n) for n in names]
    imgs = [np.array(Image.open(p).convert("RGB")) for p in paths]
    results = []
    for middle in (CAPTIONS[1], "restore the image cleanly"):
        (tmp_path / "caps.json").write_text(json.dumps({"a.png": CAPTIONS[0], "sub/b.png": middle, "c.png": CAPTIONS[3]}))
        src = TP.PromptSource(tok, TP.DeviceBackend(enc, 20, 4, 3), 20, TP.CaptionLookup(str(tmp_path / "caps.json"), str(tmp_path / "in")))
        src.set_fixed(y.cuda(), mask3.cuda())
        first = src.batch(paths)
        assert first[0].text_prompt_key == (("caption", CAPTIONS[0]), ("caption", middle), ("caption", CAPTIONS[3].strip())) and src.batch([str(tmp_path / "in" / "x.png")])[0].text_prompt_key == (("fixed", 1),)
        # the same batch twice: the second one's key is the first one's, so it sets nothing and has to give the same images
        out = list(process_stream(dit, [(imgs, *first), (imgs, *src.batch(paths))], "wavelet", False, False, 512, 448, preprocess_model=sw, vae=vae, y=y.cuda(),
                                  y_mask=mask3.cuda()))
        src.finish()
        assert src.encoded == 3 and all(np.array_equal(p, q) for p, q in zip(out[0][0], out[1][0]))
        results.append(out[0][0])
    (a0, b0, c0), (a1, b1, c1) = results
    assert np.array_equal(a0, a1) and np.array_equal(c0, c1)
    assert not np.array_equal(b0, b1), "the caption did not reach the network"


def test_device_triples_without_the_marker_keep_the_host_route_and_equal_captions_take_one_slot(tmp_path, t5):
    """process_stream's documented triples are untouched: y [n, T, C] with the command line's mask [1, 1, T], both on the device, still goes through
    prompt_bias (one mask row for every prompt) and gives what the same tensors on the host give. Only a batch PromptSource.batch() marked takes the
    device route, and there equal captions share one prompt slot - the images of n slots."""
    from instarevive_amd import text_prompts as TP
    from instarevive_amd.pipeline import process_stream
    from tests import test_models_gpu as M
    tok, enc = t5
    (sw, _), (vae, _), (dit, _) = M._small_models()
    y1, mask3 = M._prompt(M.DIT_SMALL)
    imgs = [(det_input(580 + i, (64, 64, 3)) * 255).numpy().astype(np.uint8) for i in range(3)]
    y3 = det_input(77, (3, 20, 64), -1, 1)
    run = lambda batches: [o[0] for o in process_stream(dit, batches, "wavelet", False, False, 512, 448, preprocess_model=sw, vae=vae, y=y1.cuda(), y_mask=mask3.cuda())]
    host, dev = run([(imgs, y3, mask3)]), run([(imgs, y3.cuda(), mask3.cuda())])
    assert not hasattr(y3, "text_prompt_key") and all(np.array_equal(p, q) for p, q in zip(host[0], dev[0]))
    assert not np.array_equal(host[0][0], run([(imgs, y3[[1, 0, 2]].contiguous().cuda(), mask3.cuda())])[0][0])   # the prompts are per image
    # one caption for the whole batch: the marked batch sets one slot; the same prompts through the host route (three equal rows, collapsed there too)
    names = _inputs(tmp_path / "in", [(64, 64)] * 3, 590)
    paths = [str(tmp_path / "in" / n) for n in names]
    (tmp_path / "caps.json").write_text(json.dumps({os.path.basename(n): CAPTIONS[1] for n in names}))
    src = TP.PromptSource(tok, TP.DeviceBackend(enc, 20, 4, 3), 20, TP.CaptionLookup(str(tmp_path / "caps.json"), str(tmp_path / "in")))
    src.set_fixed(y1.cuda(), mask3.cuda())
    yb, mb = src.batch(paths)
    assert len(set(yb.text_prompt_key)) == 1 and tuple(yb.shape) == (3, 20, 64) and src.encoded == 1
    marked, plain = run([(imgs, yb, mb)]), run([(imgs, yb.cpu().clone(), mb.cpu().clone())])
    assert all(np.array_equal(p, q) for p, q in zip(marked[0], plain[0]))
    src.finish()


# ------------------------------------------------------------------------------------------------ 7. ids outside the vocabulary
def test_bad_ids_are_refused_on_the_host_and_flagged_not_read_on_the_device(t5):
    from instarevive_amd import _lib as L
    from instarevive_amd import text_prompts as TP
    tok, enc = t5
    vocab, T = enc.cfg["vocab_size"], 24
    ids, mask = TP.tokenize(tok, [CAPTIONS[0], CAPTIONS[1]], T)
    bad = ids.clone()
    bad[0, 2], bad[1, 0], bad[1, 5] = vocab, -7, 2 ** 30
    # the host check: nothing is uploaded, nothing is encoded
    be = TP.DeviceBackend(enc, T, 2, 2)
    with pytest.raises(TP.TextPromptError, match="outside the encoder's vocabulary"):
        be.encode_store(bad, mask, [0, 1])
    with pytest.raises(TP.TextPromptError):
        be.encode_fp32(bad[:1], mask[:1])
    assert enc.status() == 0
    # past the host check, through the raw entry point: the call returns 0, the lookup reads row 0 in place of the bad ids, the status word says so
    out = torch.empty(2, T, CFG["d_model"], device="cuda")
    enc.encode_prompts(bad.to("cuda", torch.int32), mask.to("cuda", torch.float32), out)
    torch.cuda.synchronize()
    assert enc.status(clear=False) == L.T5_STATUS_BAD_ID and enc.status() == L.T5_STATUS_BAD_ID and enc.status() == 0   # sticky until cleared
    row0 = bad.clone()
    row0[(bad < 0) | (bad >= vocab)] = 0
    want = enc(input_ids=row0, attention_mask=mask)["last_hidden_state"]       # ir_t5_encode keeps its own flag: it is not tripped by the word above
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and bool(torch.isfinite(out).all())
    # a slot outside the cache reads nothing from it: it takes the fixed prompt and sets the other bit
    cache, cmask = torch.ones(2, T, 64, dtype=torch.float16, device="cuda"), torch.ones(2, T, device="cuda")
    fixed, fmask = torch.full((T, 64), 5.0, device="cuda"), torch.zeros(T, device="cuda")
    y, bias = _gather(enc.ctx, cache, cmask, [1, 2, 2 ** 30], fixed, fmask)   # (the status word lives in the encoder's context)
    assert bool((y[0] == 1).all()) and bool((y[1:] == 5).all()) and bool((bias[0] == 1).all()) and bool((bias[1:] == 0).all())
    assert enc.status() == L.T5_STATUS_BAD_SLOT and enc.status() == 0
