"""Prompts typed as text, encoded inside the run: --prompt TEXT and --captions PATH of inference.py / eval_batch.py.

The reference encodes captions offline (tools/extract_caption.py:136-165: T5Tokenizer(max_length, padding="max_length", truncation) ->
T5EncoderModel -> `<stem>.npz` with caption_feature fp16 [1, T, C] and attention_mask int16 [1, T]) and its fixed prompt with a training-side helper
(test_scripts/test_controlnet.py:383-395 -> .pth with fp32 embeddings). Here the same tokenizer class feeds the HIP T5 encoder behind the network:

  * PromptSource offers the prompt() / batch() surface of prompts.Captions and returns DEVICE tensors: the captions of a batch that are not
    cached yet are encoded with ir_t5_encode_prompts (stream-ordered, no host wait), stored in a device-resident cache keyed by the cleaned
    caption string (ir_prompt_cache_store: fp16, the rounding of the reference's npz files), and the batch's block for ir_dit_set_prompts
    is assembled in one launch (ir_prompt_gather). An image without a caption takes the fixed prompt.
  * the fixed prompt of --prompt keeps the encoder's fp32 output, as the .pth producer does (tools/make_prompt.py writes the same bits).
  * CaptionLookup finds an image's caption in a {file name: caption} JSON (extract_caption.py's --t5_json_path) or a folder of <stem>.txt files.
  * save_caption() writes the reference's npz file; prompts.load_caption reads it back to the bits the cache holds.

Every prompt of a run has the same token count T (prompts.py: the reference adds its 3-D mask to the scores instead of masking the padding out,
so a padded prompt would change results). The mask row travels as the values 1 / 0 it holds, exactly as the file routes pass it.
"""
import json
import os
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .prompts import CaptionError

DEFAULT_MAX_LENGTH = 300   # the reference's prompt files (inference.py:12: caption_embeds [1, 300, 4096])


class TextPromptError(CaptionError):
    pass


# ------------------------------------------------------------------------------------------------ flags (shared by both command lines)
def add_flags(parser) -> None:
    parser.add_argument("--prompt", type=str, default=None, metavar="TEXT", help="the run's fixed prompt as text: tokenised and T5-encoded at start-up (fp32, the "
                        "bits tools/make_prompt.py would write for --prompt_embeds), then the encoder is released unless --captions needs it. Needs --t5 or "
                        "--t5_pipeline; not together with a --prompt_embeds of your own")
    parser.add_argument("--captions", type=str, default=None, metavar="PATH", help="per-image prompts as text, T5-encoded on the device inside the run: a JSON "
                        "file {file name: caption} (the reference's tools/extract_caption.py --t5_json_path; keys are matched by input-relative path, then base "
                        "name, then stem) or a folder of <stem>.txt files (DIR/<input-relative path without extension>.txt, else DIR/<file stem>.txt). A "
                        "repeated caption is encoded once. Images without one get --prompt, else --prompt_embeds. Needs --t5 or --t5_pipeline; not together "
                        "with --caption_dir")
    parser.add_argument("--t5", type=str, default=None, metavar="DIR", help="folder with the T5 tokenizer files and encoder weights (DeepFloyd/t5-v1_1-xxl layout)")
    parser.add_argument("--t5_pipeline", type=str, default=None, metavar="DIR", help="diffusers pipeline folder with tokenizer/ and text_encoder/ subfolders (PixArt-XL-2-*)")
    parser.add_argument("--prompt_max_length", type=int, default=None, metavar="N", help="token count T of every prompt of the run (padding=\"max_length\", "
                        "truncation); default: the T of the fixed prompt file, or 300 with --prompt")
    parser.add_argument("--clean_captions", action="store_true", help="apply the reference's caption cleaning (T5Embedder.text_preprocessing) to --prompt and --captions first")
    parser.add_argument("--save_captions", type=str, default=None, metavar="DIR", help="with --captions: write every encoded caption as the reference's file "
                        "DIR/<input-relative path without extension>.npz (caption_feature fp16 [1, T, C], attention_mask int16 [1, T]), readable by "
                        "--caption_dir and by the reference's datasets")


def check_flags(args, default_prompt_embeds: str) -> Optional[str]:
    """The one-line refusal of a flag combination, or None. Called before anything loads."""
    text = args.prompt is not None or args.captions is not None
    if args.captions is not None and getattr(args, "caption_dir", None):
        return "--captions is not offered together with --caption_dir (one source of per-image prompts per run)"
    if args.prompt is not None and args.prompt_embeds != default_prompt_embeds:
        return "--prompt is not offered together with --prompt_embeds (one fixed prompt per run)"
    if text and bool(args.t5) == bool(args.t5_pipeline):
        return "--prompt / --captions need the T5 folder: give exactly one of --t5 DIR / --t5_pipeline DIR"
    if not text and (args.t5 or args.t5_pipeline or args.prompt_max_length is not None or args.clean_captions or args.save_captions):
        return "--t5 / --t5_pipeline / --prompt_max_length / --clean_captions / --save_captions belong to --prompt / --captions: give one of them"
    if args.save_captions and args.captions is None:
        return "--save_captions writes the captions --captions encodes: give --captions as well"
    if args.prompt_max_length is not None and not 1 <= args.prompt_max_length <= 512:
        return "--prompt_max_length: the T5 encoder takes 1 .. 512 tokens"
    if args.captions is not None and not os.path.exists(args.captions):
        return f"--captions {args.captions}: no such file or folder"
    return None


# ------------------------------------------------------------------------------------------------ tokenizer / encoder
def load_tokenizer(t5: Optional[str] = None, t5_pipeline: Optional[str] = None):
    """transformers' T5Tokenizer from a LOCAL folder, exactly as tools/make_prompt.py loads it."""
    from transformers import T5Tokenizer
    if bool(t5) == bool(t5_pipeline):
        raise TextPromptError("give exactly one of t5 / t5_pipeline")
    return T5Tokenizer.from_pretrained(t5_pipeline, subfolder="tokenizer") if t5_pipeline else T5Tokenizer.from_pretrained(t5)


def load_encoder(device, t5: Optional[str] = None, t5_pipeline: Optional[str] = None):
    from .models import T5EncoderModel
    enc = T5EncoderModel.from_pretrained(t5_pipeline, subfolder="text_encoder") if t5_pipeline else T5EncoderModel.from_pretrained(t5)
    return enc.to(torch.device(device))


def tokenize(tokenizer, texts: Sequence[str], max_length: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids int64 [b, T], mask int64 [b, T]) as the reference's producers make them: padded to max_length, a longer caption truncated."""
    tok = tokenizer(list(texts), max_length=max_length, padding="max_length", truncation=True, return_tensors="pt")
    return tok["input_ids"], tok["attention_mask"]


def check_ids(ids: torch.Tensor, vocab: int) -> None:
    """The host's refusal of an id outside the encoder's vocabulary, before anything is uploaded."""
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= vocab:
        raise TextPromptError(f"token id {lo if lo < 0 else hi} is outside the encoder's vocabulary [0, {vocab}): the tokenizer and the encoder weights do not belong together")


def clean(text: str, on: bool) -> str:
    if not on:
        return text
    from .captions import text_preprocessing
    return text_preprocessing(text)


# ------------------------------------------------------------------------------------------------ caption lookup
class CaptionLookup:
    """The caption text of an image, or None. JSON: {file name: caption}, keys matched by input-relative path, then base name, then stem (each with and
    without the extension the key carries). Folder: `<dir>/<input-relative path without extension>.txt`, then `<dir>/<file stem>.txt` - the two-step search
    of prompts.caption_file. Captions are stripped of surrounding white space, as the reference's producer does (extract_caption.py:150)."""

    def __init__(self, path: str, input_root: Optional[str] = None):
        self.path, self.input_root = path, input_root
        self.table = None
        if os.path.isdir(path):
            return
        try:
            with open(path, encoding="utf-8") as f:
                table = json.load(f)
        except (OSError, ValueError) as e:
            raise TextPromptError(f"{path}: not a caption JSON ({e})") from e
        if not isinstance(table, dict) or not all(isinstance(v, str) for v in table.values()):
            raise TextPromptError(f"{path}: a caption JSON is one object {{file name: caption}}")
        self.table = {k.replace("\\", "/"): v for k, v in table.items()}
        self.by_base, self.by_stem = {}, {}
        for k, v in self.table.items():   # the first key of a base name / stem wins, in the file's order
            base = os.path.basename(k)
            self.by_base.setdefault(base, v)
            self.by_stem.setdefault(os.path.splitext(base)[0], v)

    def rel(self, image_path: str) -> Optional[str]:
        if self.input_root is None:
            return None
        rel = os.path.relpath(image_path, self.input_root)
        return None if rel.startswith("..") else rel.replace(os.sep, "/")

    def find(self, image_path: str) -> Optional[str]:
        base = os.path.basename(image_path)
        stem = os.path.splitext(base)[0]
        rel = self.rel(image_path)
        if self.table is not None:
            if rel is not None:
                for k in (rel, os.path.splitext(rel)[0]):
                    if k in self.table:
                        return self.table[k].strip()
            for k, index in ((base, self.by_base), (stem, self.by_stem)):   # a key that IS the name wins over a longer key that ends in it
                if k in self.table:
                    return self.table[k].strip()
                if k in index:
                    return index[k].strip()
            return None
        cands = [os.path.join(self.path, os.path.splitext(rel)[0] + ".txt")] if rel is not None else []
        cands.append(os.path.join(self.path, stem + ".txt"))
        for c in cands:
            if os.path.isfile(c):
                with open(c, encoding="utf-8") as f:
                    return f.read().strip()
        return None

    def __len__(self):
        if self.table is not None:
            return len(self.table)
        return sum(f.endswith(".txt") for _, _, fs in os.walk(self.path) for f in fs)


# ------------------------------------------------------------------------------------------------ the reference's caption file
def caption_path(save_dir: str, image_path: str, input_root: Optional[str] = None) -> str:
    """Where the caption file of an image goes: `save_dir/<input-relative path without extension>.npz` (what prompts.caption_file looks for first)."""
    rel = os.path.relpath(image_path, input_root) if input_root is not None else os.path.basename(image_path)
    if rel.startswith(".."):
        rel = os.path.basename(image_path)
    return os.path.join(save_dir, os.path.splitext(rel)[0] + ".npz")


def save_caption(path: str, feature: torch.Tensor, mask: torch.Tensor) -> None:
    """The reference's file (extract_caption.py:160-165): caption_feature fp16 [1, T, C], attention_mask int16 [1, T], np.savez_compressed."""
    f = feature.detach().to("cpu")
    f = f.reshape(1, f.shape[-2], f.shape[-1])
    f = (f if f.dtype == torch.float16 else f.to(torch.float16)).contiguous().numpy()
    m = mask.detach().to("cpu").reshape(1, -1).to(torch.int16).contiguous().numpy()
    if m.shape[1] != f.shape[1]:
        raise TextPromptError(f"{path}: a mask of {m.shape[1]} entries for {f.shape[1]} tokens")
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    np.savez_compressed(path, caption_feature=f, attention_mask=m)


# ------------------------------------------------------------------------------------------------ device side
class DeviceBackend:
    """What PromptSource does on the GPU: the encoder, the cache of encoded captions and the gather. Everything a batch queues is stream-ordered on
    the current stream; only read_slot() (for --save_captions) and status() wait."""

    def __init__(self, encoder, tokens: int, capacity: int, max_batch: int, fp16: bool = True):
        self.enc, self.ctx, self.device = encoder, encoder.ctx, encoder.device
        self.tokens, self.dim, self.capacity, self.max_batch, self.fp16 = tokens, encoder.cfg["d_model"], capacity, max(max_batch, 1), fp16
        self.vocab = encoder.cfg["vocab_size"]
        encoder.prepare(self.max_batch, tokens)   # the position-bias table of this T and the workspace: nothing is allocated on first use
        self.cache = torch.zeros(capacity, tokens, self.dim, dtype=torch.float16 if fp16 else torch.float32, device=self.device)
        self.cache_mask = torch.zeros(capacity, tokens, dtype=torch.float32, device=self.device)
        self.out = torch.empty(self.max_batch, tokens, self.dim, dtype=torch.float32, device=self.device)
        self.fixed = None

    def _upload(self, ids, mask):
        check_ids(ids, self.vocab)
        hi, hm = ids.to(torch.int32).contiguous().pin_memory(), mask.to(torch.float32).contiguous().pin_memory()
        return hi.to(self.device, non_blocking=True), hm.to(self.device, non_blocking=True)

    def encode_fp32(self, ids, mask):
        """The fixed prompt's route: (y fp32 [b, T, C], mask fp32 [b, T]) on the device, the encoder's output as it is. Called once per run: it
        allocates its output and prepares the encoder for its batch size on every call."""
        di, dm = self._upload(ids, mask)
        out = torch.empty(ids.shape[0], self.tokens, self.dim, dtype=torch.float32, device=self.device)
        self.enc.prepare(ids.shape[0], self.tokens)
        self.enc.encode_prompts(di, dm, out)
        return out, dm

    def encode_store(self, ids, mask, slots: Sequence[int]) -> None:
        """Encode b <= max_batch captions and store caption j in cache slot slots[j] (one store launch per run of consecutive slots)."""
        b = ids.shape[0]
        di, dm = self._upload(ids, mask)
        self.enc.encode_prompts(di, dm, self.out[:b])
        lib, j = self.ctx.lib, 0
        while j < b:
            r = 1
            while j + r < b and slots[j + r] == slots[j] + r:
                r += 1
            self.ctx.check(lib.ir_prompt_cache_store(self.ctx.h, self.ctx.stream(), L.ptr(self.out[j:j + r]), L.ptr(dm[j:j + r]), L.ptr(self.cache), L.ptr(self.cache_mask),
                                                     int(self.fp16), self.capacity, slots[j], r, self.tokens, self.dim), "ir_prompt_cache_store")
            j += r

    def set_fixed(self, y, mask) -> None:
        self.fixed = (y.detach().to(self.device, torch.float32).reshape(self.tokens, self.dim).contiguous(),
                      mask.detach().to(self.device, torch.float32).reshape(self.tokens).contiguous())

    def gather(self, slots: Sequence[int]):
        """(y fp32 [n, T, C], bias fp32 [n, T]) of a batch: cache slot slots[i], or the fixed prompt for a negative slot. The two results come from
        torch's caching allocator per batch (the DiT keeps the previous batch's until its K / V are rebuilt), the slot list through pinned memory."""
        n = len(slots)
        ds = torch.tensor(list(slots), dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        y = torch.empty(n, self.tokens, self.dim, dtype=torch.float32, device=self.device)
        bias = torch.empty(n, self.tokens, dtype=torch.float32, device=self.device)
        self.ctx.check(self.ctx.lib.ir_prompt_gather(self.ctx.h, self.ctx.stream(), L.ptr(self.cache), L.ptr(self.cache_mask), int(self.fp16), self.capacity, L.ptr(ds),
                                                     L.ptr(self.fixed[0]), L.ptr(self.fixed[1]), L.ptr(y), L.ptr(bias), n, self.tokens, self.dim), "ir_prompt_gather")
        return y, bias

    def read_slot(self, slot: int):
        return self.cache[slot].to("cpu"), self.cache_mask[slot].to("cpu")

    def resident_bytes(self) -> int:
        return self.enc.resident_bytes()

    def status(self) -> int:
        return self.enc.status()

    def release_encoder(self) -> None:
        self.enc.release()
        self.out = None


class PromptSource:
    """The prompts of a run from text. prompt() / batch() as prompts.Captions offers them, on the device.

    tokenizer: transformers' T5Tokenizer (or anything with its call surface); backend: a DeviceBackend; lookup: a CaptionLookup or None;
    fixed prompt: set_fixed_text() (encoded, fp32) or set_fixed() (the --prompt_embeds tensors)."""

    def __init__(self, tokenizer, backend, max_length: int, lookup: Optional[CaptionLookup] = None, clean_captions: bool = False,
                 save_dir: Optional[str] = None, input_root: Optional[str] = None):
        self.tokenizer, self.backend, self.n_tok, self.lookup = tokenizer, backend, max_length, lookup
        self.clean_captions, self.save_dir, self.input_root = clean_captions, save_dir, input_root
        self.slots = OrderedDict()   # cleaned caption -> cache slot, least recently used first
        self.free = list(range(backend.capacity - 1, -1, -1))
        self.encoded = 0             # captions that went through the encoder (a repeated caption counts once while it stays cached)
        self.saved = set()
        self.host = {}               # --save_captions: the host copy of a cached caption, fetched once however many files share it
        self.fb_y = self.fb_m = None
        self.fixed_version = 0

    # ---- the fixed prompt
    def set_fixed(self, y: torch.Tensor, mask: torch.Tensor) -> None:
        y = y.reshape(-1, y.shape[-2], y.shape[-1])[0]
        mask = mask.reshape(-1, mask.shape[-1])[0]
        if y.shape[0] != self.n_tok or mask.shape[0] != self.n_tok:
            raise TextPromptError(f"the fixed prompt has {y.shape[0]} tokens, the run's prompts have {self.n_tok} (--prompt_max_length; every prompt of a run "
                                  f"needs the same token count: padding would change results)")
        self.backend.set_fixed(y, mask)
        self.fb_y, self.fb_m = self.backend.fixed
        self.fixed_version += 1

    def set_fixed_text(self, text: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """Encode the run's fixed prompt (fp32, as tools/make_prompt.py saves it) and make it the fallback. -> (y [1, T, C], mask [1, T]) on the device."""
        ids, mask = tokenize(self.tokenizer, [clean(text, self.clean_captions)], self.n_tok)
        y, m = self.backend.encode_fp32(ids, mask)
        self.set_fixed(y, m)
        return y, m

    # ---- per-image captions
    def caption(self, image_path: str) -> Optional[str]:
        """The cleaned caption of an image (the cache's key), or None for an image without one."""
        text = self.lookup.find(image_path) if self.lookup is not None else None
        return None if text is None else clean(text, self.clean_captions)

    def _ensure(self, captions: Sequence[str]) -> None:
        """Every caption of the list cached: the missing ones are encoded, in the list's order, max_batch at a time."""
        need = list(OrderedDict.fromkeys(captions))
        if len(need) > self.backend.capacity:
            raise TextPromptError(f"a batch of {len(need)} different captions does not fit a cache of {self.backend.capacity} slots")
        for c in need:
            if c in self.slots:
                self.slots.move_to_end(c)
        missing = [c for c in need if c not in self.slots]
        for c in missing:
            if self.free:
                self.slots[c] = self.free.pop()
            else:   # the least recently used caption that this batch does not need
                victim = next(k for k in self.slots if k not in need)
                self.slots[c] = self.slots.pop(victim)
                self.host.pop(victim, None)
        for i in range(0, len(missing), self.backend.max_batch):
            part = missing[i:i + self.backend.max_batch]
            ids, mask = tokenize(self.tokenizer, part, self.n_tok)
            self.backend.encode_store(ids, mask, [self.slots[c] for c in part])
            self.encoded += len(part)

    def _save(self, image_path: str, caption: str) -> None:
        path = caption_path(self.save_dir, image_path, self.input_root)
        if path not in self.saved:
            self.saved.add(path)
            if caption not in self.host:   # the one wait on the stream a caption costs, while it stays cached
                self.host[caption] = self.backend.read_slot(self.slots[caption])
            save_caption(path, *self.host[caption])

    def _slots_of(self, image_paths: Sequence[str]):
        """(cache slot per image, -1 for the fixed prompt; the cleaned captions, None for an image without one)."""
        if self.fb_y is None:
            raise TextPromptError("PromptSource: no fixed prompt set (set_fixed / set_fixed_text)")
        caps = [self.caption(p) for p in image_paths]
        self._ensure([c for c in caps if c is not None])
        if self.save_dir:
            for p, c in zip(image_paths, caps):
                if c is not None:
                    self._save(p, c)
        return [-1 if c is None else self.slots[c] for c in caps], caps

    def prompt(self, image_path: str):
        """(y [T, C], mask [T], caption or None) of one image, on the device."""
        (slot,), (cap,) = self._slots_of([image_path])
        if slot < 0:
            return self.fb_y, self.fb_m, None
        y, bias = self.backend.gather([slot])
        return y[0], bias[0], cap

    def batch(self, image_paths: Sequence[str]):
        """(y [B, T, C], y_mask [B, 1, T]) of a batch of images, in order, on the device. y carries `text_prompt_key`, one entry per image that
        names the prompt's content (the caption, or the fixed prompt's version): process_stream() takes a batch marked so straight from the
        device, sets equal prompts as one slot and sets nothing when the key is the previous batch's."""
        slots, caps = self._slots_of(image_paths)
        y, bias = self.backend.gather(slots)
        y.text_prompt_key = tuple(("fixed", self.fixed_version) if c is None else ("caption", c) for c in caps)
        return y, bias[:, None, :]

    # ---- end of the run
    def finish(self) -> None:
        """The device's status word at the end of the run: an id outside the vocabulary, or a slot outside the cache, that got past the host checks."""
        word = self.backend.status()
        if word:
            raise TextPromptError(f"the text prompt path reported status {word} ({'an id outside the vocabulary' if word & L.T5_STATUS_BAD_ID else 'a slot outside the cache'} "
                                  f"reached the device): the results of this run are not to be trusted")


def fixed_prompt_length(prompt_embeds_path: str) -> int:
    return int(torch.load(prompt_embeds_path, map_location="cpu")["caption_embeds"].shape[-2])


def setup(args, m, device, log=print, max_batch: int = 1) -> Optional[PromptSource]:
    """The command lines' set-up after load_models(): encodes --prompt into m.y / m.y_mask, and returns the PromptSource of --captions (else None).
    The encoder is loaded once; with --prompt alone it is released after its single encode."""
    if args.prompt is None and args.captions is None:
        return None
    tokenizer = load_tokenizer(args.t5, args.t5_pipeline)
    enc = load_encoder(device, args.t5, args.t5_pipeline)
    width = m.model.cfg["caption_channels"]
    if enc.cfg["d_model"] != width:
        raise SystemExit(f"--t5 / --t5_pipeline: the encoder's d_model {enc.cfg['d_model']} is not the network's caption width {width}")
    n_tok = args.prompt_max_length or (DEFAULT_MAX_LENGTH if args.prompt is not None else int(m.y.shape[-2]))
    lookup = CaptionLookup(args.captions, args.input) if args.captions is not None else None
    capacity = max(min(len(lookup), 256), 2 * max_batch, 1) if lookup is not None else 1
    backend = DeviceBackend(enc, n_tok, capacity, max_batch if lookup is not None else 1)
    log(f"text prompts: T5 encoder resident, {backend.resident_bytes() / 1e9:.2f} GB of weights; T = {n_tok}"
        + (f"; caption cache {capacity} slots = {backend.cache.numel() * 2 / 1e6:.1f} MB" if lookup is not None else ""))
    src = PromptSource(tokenizer, backend, n_tok, lookup, args.clean_captions, args.save_captions, args.input)
    try:
        if args.prompt is not None:
            y, mask = src.set_fixed_text(args.prompt)
            m.y, m.y_mask = y.reshape(1, n_tok, -1), mask.reshape(1, 1, n_tok)
        else:
            src.set_fixed(m.y, m.y_mask)
    except CaptionError as e:
        raise SystemExit(f"--prompt / --captions: {e}")
    if lookup is None:
        src.finish()
        backend.release_encoder()
        log("text prompts: --prompt encoded, the encoder's memory is released")
        return None
    return src
