"""Prompts as text (--prompt / --captions), the host side without a GPU: caption lookup, the fallback chain, the caption cache's bookkeeping,
the reference's npz file, the command lines' refusals, the exported symbols, and what the tokenizer does to long and empty captions."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, DIM = 12, 8


@pytest.fixture(scope="module")
def tokenizer(tmp_path_factory):
    import sentencepiece as spm
    from transformers import T5Tokenizer
    d = tmp_path_factory.mktemp("t5tok")
    corpus = d / "corpus.txt"
    corpus.write_text("\n".join(["a high quality photo of a human face", "highly detailed portrait, sharp focus, 8k", "restore the image cleanly",
                                 "a photo of a cat and a dog in the garden", "clean, realistic, natural skin texture"] * 4))
    spm.SentencePieceTrainer.train(input=str(corpus), model_prefix=str(d / "spiece"), vocab_size=60, model_type="unigram", pad_id=0, eos_id=1, unk_id=2,
                                   bos_id=-1, hard_vocab_limit=False, minloglevel=2)
    os.remove(corpus)
    return T5Tokenizer.from_pretrained(str(d))


class FakeBackend:
    """DeviceBackend's surface on the host: an "encoding" of a caption is its ids as floats, so what a slot holds says which caption went there."""

    def __init__(self, capacity=4, max_batch=2):
        self.capacity, self.max_batch, self.fixed = capacity, max_batch, None
        self.cache = torch.zeros(capacity, T, DIM)
        self.cache_mask = torch.zeros(capacity, T)
        self.calls = []

    def _enc(self, ids):
        return ids.to(torch.float32)[:, :, None].expand(-1, -1, DIM).contiguous()

    def encode_fp32(self, ids, mask):
        self.calls.append(("fixed", ids.shape[0]))
        return self._enc(ids), mask.to(torch.float32)

    def encode_store(self, ids, mask, slots):
        assert ids.shape[0] <= self.max_batch and len(slots) == ids.shape[0]
        self.calls.append(("store", list(slots)))
        for j, s in enumerate(slots):
            self.cache[s], self.cache_mask[s] = self._enc(ids)[j], mask[j].to(torch.float32)

    def set_fixed(self, y, mask):
        self.fixed = (y.reshape(T, DIM).to(torch.float32), mask.reshape(T).to(torch.float32))

    def gather(self, slots):
        y = torch.stack([self.fixed[0] if s < 0 else self.cache[s] for s in slots])
        b = torch.stack([self.fixed[1] if s < 0 else self.cache_mask[s] for s in slots])
        return y, b

    def read_slot(self, slot):
        return self.cache[slot].to(torch.float16), self.cache_mask[slot]

    def status(self):
        return 0


def _tree(tmp_path):
    root = tmp_path / "in"
    (root / "sub").mkdir(parents=True)
    files = [root / "a.png", root / "sub" / "a.png", root / "sub" / "b.jpg", root / "c.png"]
    for f in files:
        f.write_bytes(b"x")
    return root, [str(f) for f in files]


def test_json_lookup_order_relative_path_then_base_name_then_stem(tmp_path):
    from instarevive_amd.text_prompts import CaptionLookup, TextPromptError
    root, (a, sub_a, sub_b, c) = _tree(tmp_path)
    table = {"sub/a.png": " the nested a ", "a.png": "a by base name", "b": "b by stem", "other/c.png": "c by another folder's base name"}
    (tmp_path / "caps.json").write_text(json.dumps(table))
    look = CaptionLookup(str(tmp_path / "caps.json"), str(root))
    assert look.find(sub_a) == "the nested a"            # the input-relative path wins over the base name, and captions are stripped
    assert look.find(a) == "a by base name"              # relative path "a.png" = the key
    assert look.find(sub_b) == "b by stem"               # no "sub/b.jpg", no "b.jpg": the stem
    assert look.find(c) == "c by another folder's base name"
    assert look.find(str(root / "none.png")) is None and len(look) == 4
    # without an input root only base name and stem are tried
    assert CaptionLookup(str(tmp_path / "caps.json")).find(sub_a) == "a by base name"
    (tmp_path / "bad.json").write_text("[1, 2]")
    with pytest.raises(TextPromptError):
        CaptionLookup(str(tmp_path / "bad.json"))


def test_txt_lookup_is_the_two_step_search_of_caption_file(tmp_path):
    from instarevive_amd.text_prompts import CaptionLookup
    root, (a, sub_a, sub_b, c) = _tree(tmp_path)
    caps = tmp_path / "caps"
    (caps / "sub").mkdir(parents=True)
    (caps / "sub" / "a.txt").write_text("nested a\n")
    (caps / "a.txt").write_text("flat a")
    (caps / "b.txt").write_text("flat b")
    (caps / "c.txt").write_text("")
    look = CaptionLookup(str(caps), str(root))
    assert look.find(sub_a) == "nested a" and look.find(a) == "flat a" and look.find(sub_b) == "flat b"
    assert look.find(c) == ""                             # an empty file is an empty caption, not a missing one
    assert look.find(str(root / "d.png")) is None and len(look) == 4


def test_fallback_chain_and_the_cache_encodes_a_repeated_caption_once(tmp_path, tokenizer):
    from instarevive_amd.text_prompts import CaptionLookup, PromptSource, TextPromptError, tokenize
    root, (a, sub_a, sub_b, c) = _tree(tmp_path)
    (tmp_path / "caps.json").write_text(json.dumps({"sub/a.png": "a photo of a cat", "a.png": "a photo of a cat", "b.jpg": "a dog in the garden"}))
    look = CaptionLookup(str(tmp_path / "caps.json"), str(root))
    be = FakeBackend(capacity=2, max_batch=2)
    src = PromptSource(tokenizer, be, T, look)
    with pytest.raises(TextPromptError):
        src.batch([a])                                    # no fixed prompt yet
    # --prompt_embeds is the fallback when no --prompt was given ...
    fy, fm = torch.full((1, T, DIM), 7.0), torch.ones(1, 1, T)
    src.set_fixed(fy, fm)
    y, m = src.batch([a, c, sub_a, sub_b])
    assert tuple(y.shape) == (4, T, DIM) and tuple(m.shape) == (4, 1, T)
    ids, mask = tokenize(tokenizer, ["a photo of a cat", "a dog in the garden"], T)
    assert torch.equal(y[0, :, 0], ids[0].float()) and torch.equal(y[2], y[0]) and torch.equal(y[3, :, 0], ids[1].float())
    assert torch.equal(y[1], fy[0]) and torch.equal(m[1, 0], fm[0, 0]) and torch.equal(m[0, 0], mask[0].float())
    assert src.encoded == 2 and be.calls == [("store", [0, 1])]          # three captioned images, two different captions, one encoder call
    src.batch([sub_a, a])
    assert src.encoded == 2 and len(be.calls) == 1                        # cached: nothing is encoded again
    assert src.prompt(c)[2] is None and src.prompt(a)[2] == "a photo of a cat" and torch.equal(src.prompt(a)[0], y[0])
    # ... and --prompt replaces it: an image without a caption then gets the encoded text
    y1, m1 = src.set_fixed_text("restore the image cleanly")
    want, wmask = tokenize(tokenizer, ["restore the image cleanly"], T)
    assert be.calls[-1] == ("fixed", 1) and torch.equal(y1[0, :, 0], want[0].float()) and torch.equal(src.batch([c])[0][0, :, 0], want[0].float())
    # a third caption evicts the least recently used one that the batch does not need; a batch that cannot fit is refused
    look.table["c.png"] = "sharp focus"
    look.by_base["c.png"] = "sharp focus"
    src.batch([sub_b, c])
    assert src.encoded == 3 and "a photo of a cat" not in src.slots and set(src.slots) == {"a dog in the garden", "sharp focus"}
    src.batch([a])
    assert src.encoded == 4                                               # evicted, so encoded again
    with pytest.raises(TextPromptError):
        src.batch([a, sub_b, c])
    # a fixed prompt of another token count is refused: every prompt of a run has the same T
    with pytest.raises(TextPromptError):
        src.set_fixed(torch.zeros(1, T + 1, DIM), torch.ones(1, 1, T + 1))


def test_saved_caption_file_is_the_reference_format_and_loads_through_load_caption(tmp_path, tokenizer):
    from instarevive_amd import prompts
    from instarevive_amd.text_prompts import CaptionLookup, PromptSource, caption_path, save_caption
    feat = torch.randn(T, DIM) * 3
    mask = torch.tensor([1.0] * 5 + [0.0] * (T - 5))
    path = str(tmp_path / "out" / "sub" / "x.npz")
    save_caption(path, feat, mask)
    with np.load(path) as z:
        assert sorted(z.files) == ["attention_mask", "caption_feature"]
        assert z["caption_feature"].dtype == np.float16 and z["caption_feature"].shape == (1, T, DIM)
        assert z["attention_mask"].dtype == np.int16 and z["attention_mask"].shape == (1, T)
        assert np.array_equal(z["caption_feature"][0], feat.to(torch.float16).numpy())
    y, m = prompts.load_caption(path)
    assert torch.equal(y, feat.to(torch.float16).float()) and torch.equal(m, mask)
    # the source writes DIR/<input-relative path without extension>.npz, once per file, where prompts.caption_file finds it
    root, (a, sub_a, sub_b, c) = _tree(tmp_path)
    (tmp_path / "caps.json").write_text(json.dumps({"a.png": "a photo of a cat"}))
    src = PromptSource(tokenizer, FakeBackend(), T, CaptionLookup(str(tmp_path / "caps.json"), str(root)), save_dir=str(tmp_path / "saved"), input_root=str(root))
    src.set_fixed(torch.zeros(1, T, DIM), torch.ones(1, 1, T))
    src.batch([sub_a, c, a])
    assert caption_path(str(tmp_path / "saved"), sub_a, str(root)) == str(tmp_path / "saved" / "sub" / "a.npz")
    assert prompts.caption_file(str(tmp_path / "saved"), sub_a, str(root)) == str(tmp_path / "saved" / "sub" / "a.npz")
    assert prompts.caption_file(str(tmp_path / "saved"), a, str(root)) == str(tmp_path / "saved" / "a.npz") and len(src.saved) == 2
    assert not os.path.exists(tmp_path / "saved" / "c.npz")
    y, m = prompts.load_caption(str(tmp_path / "saved" / "sub" / "a.npz"))
    assert tuple(y.shape) == (T, DIM) and torch.equal(y, src.batch([a])[0][0])


REFUSALS = [
    (["--captions", "CAPS", "--caption_dir", "x", "--t5", "t5"], "--captions is not offered together with --caption_dir"),
    (["--prompt", "a cat", "--prompt_embeds", "mine.pth", "--t5", "t5"], "--prompt is not offered together with --prompt_embeds"),
    (["--prompt", "a cat"], "need the T5 folder"),
    (["--captions", "CAPS"], "need the T5 folder"),
    (["--prompt", "a cat", "--t5", "a", "--t5_pipeline", "b"], "exactly one of --t5 DIR / --t5_pipeline DIR"),
    (["--save_captions", "d", "--prompt", "a cat", "--t5", "t5"], "--save_captions writes the captions --captions encodes"),
    (["--clean_captions"], "belong to --prompt / --captions"),
    (["--prompt", "a cat", "--t5", "t5", "--prompt_max_length", "513"], "1 .. 512 tokens"),
    (["--captions", "MISSING", "--t5", "t5"], "no such file or folder"),
]


@pytest.mark.parametrize("script", ["inference", "eval_batch"])
def test_command_lines_refuse_in_one_line_before_anything_loads(script, tmp_path, monkeypatch):
    """main() itself is run: a refusal has to come before a model file, a tokenizer or the GPU is touched (none of them exists here)."""
    caps = tmp_path / "caps.json"
    caps.write_text("{}")
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    mod = importlib.import_module(script)
    for extra, needle in REFUSALS:
        extra = [str(caps) if a == "CAPS" else str(tmp_path / "missing.json") if a == "MISSING" else a for a in extra]
        monkeypatch.setattr(sys, "argv", [script + ".py", "--ckpt", "none.ckpt", "--input", "in", "--output", "out"] + extra)
        with pytest.raises(SystemExit) as e:
            mod.main()
        msg = str(e.value)
        assert needle in msg and "\n" not in msg, (extra, msg)
    # without the new flags nothing is refused here, and the defaults are the ones that switch the feature off
    monkeypatch.setattr(sys, "argv", [script + ".py", "--ckpt", "none.ckpt", "--input", "in", "--output", "out"])
    a = mod.parse_args()
    cli = importlib.import_module("inference")
    cli.check_text_prompts(a)
    assert a.prompt is None and a.captions is None and a.t5 is None and a.t5_pipeline is None and a.prompt_max_length is None
    assert a.clean_captions is False and a.save_captions is None and a.caption_dir is None and a.prompt_embeds == cli.DEFAULT_PROMPT


def test_new_symbols_are_declared_and_exported():
    from instarevive_amd import _lib
    from instarevive_amd.build import build
    build()
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    for name in ("ir_t5_encode_prompts", "ir_t5_status", "ir_t5_release", "ir_prompt_cache_store", "ir_prompt_gather"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "size_t ir_t5_resident_bytes(" in header and "ir_t5_resident_bytes" in _lib.SYMBOLS and lib.ir_t5_resident_bytes(None) == 0
    assert "does not wait" in header or "never waits on the host" in header      # the stream-ordered contract is stated where the entry point is declared
    # they answer a missing context or a bad argument before anything touches a device
    assert lib.ir_t5_encode_prompts(None, None, None, None, None, 1, 8, None, 0) == -11 and lib.ir_t5_status(None, None, None, 0) == -11
    assert lib.ir_prompt_cache_store(None, None, None, None, None, None, 1, 1, 0, 1, 8, 8) == -11
    assert lib.ir_prompt_gather(None, None, None, None, 1, 0, None, None, None, None, None, 1, 8, 8) == -11
    assert _lib.T5_STATUS_BAD_ID == 1 and _lib.T5_STATUS_BAD_SLOT == 2
    for script in ("inference.py", "eval_batch.py"):
        assert "text_prompts" in open(os.path.join(ROOT, script)).read()
    assert os.path.isfile(os.path.join(ROOT, "tools", "make_captions.py"))


def test_long_caption_is_truncated_as_the_tokenizer_truncates_and_an_empty_one_is_legal(tmp_path, tokenizer):
    from instarevive_amd.text_prompts import CaptionLookup, PromptSource, TextPromptError, check_ids, tokenize
    long = "a high quality photo of a human face, highly detailed portrait, sharp focus " * 6
    ids, mask = tokenize(tokenizer, [long, "", "a cat"], T)
    want = tokenizer([long, "", "a cat"], max_length=T, padding="max_length", truncation=True, return_tensors="pt")
    assert torch.equal(ids, want["input_ids"]) and torch.equal(mask, want["attention_mask"]) and tuple(ids.shape) == (3, T)
    full = tokenizer(long)["input_ids"]
    assert len(full) > T and ids[0].tolist() == full[:T - 1] + [tokenizer.eos_token_id] and int(mask[0].sum()) == T   # cut to T - 1 pieces + EOS
    assert ids[1].tolist() == [tokenizer.eos_token_id] + [tokenizer.pad_token_id] * (T - 1) and mask[1].tolist() == [1] + [0] * (T - 1)
    # the source takes "" as a caption of its own (EOS + padding), not as "no caption"
    root, (a, sub_a, sub_b, c) = _tree(tmp_path)
    (tmp_path / "caps.json").write_text(json.dumps({"a.png": "", "c.png": long}))
    be = FakeBackend()
    src = PromptSource(tokenizer, be, T, CaptionLookup(str(tmp_path / "caps.json"), str(root)))
    src.set_fixed(torch.full((1, T, DIM), 7.0), torch.ones(1, 1, T))
    y, m = src.batch([a, c])
    assert src.encoded == 2 and torch.equal(y[0, :, 0], ids[1].float()) and torch.equal(m[0, 0], mask[1].float()) and torch.equal(y[1, :, 0], ids[0].float())
    # the host refuses ids outside the vocabulary before anything is uploaded
    check_ids(ids, len(tokenizer))
    for bad in (torch.tensor([[0, len(tokenizer)]]), torch.tensor([[-1, 3]])):
        with pytest.raises(TextPromptError):
            check_ids(bad, len(tokenizer))
