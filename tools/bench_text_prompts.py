#!/usr/bin/env python3
"""Time the text prompt path on one MI355X and write profiles/text_prompts.txt.

  1. ir_t5_encode_prompts at T5-XXL's shapes (24 layers, d_model 4096, 64 heads x 64, d_ff 10240, vocabulary 32128) and T = 300, b = 1 and b = 4:
     HIP events around the call, medians over `--repeats` timed calls over rotating ids behind `--warmup` calls, against the bf16-MFMA floor of the
     encoder's linears (derived: 2 * b * T * 24 * (3 * 4096 * 4096 + 4096 * 4096 + 2 * 4096 * 10240 + 10240 * 4096) FLOP);
  2. ir_prompt_cache_store (fp16) and ir_prompt_gather for the same batches, against the bytes they move;
  3. their share of the network step: of the 2048 x 2048 step recorded in profiles/dists.txt (115.91 ms; one prompt per image) and of the 512 x 512
     batch-of-four step that eval_batch.py runs, timed here on bench.py's seeded full-size models (process(), host pre- and post-processing included);
  4. that the encode does not wait on the host: the time the CALL takes on the host against the time the device needs for it;
  5. the command line: files/s of `inference.py --sr_scale 4 --png_encoder gpu --resize gpu --captions caps.json --t5 DIR` (one caption per file, all
     different) on this tree against `--caption_dir` over the npz files of the same captions on --baseline_root (a built checkout of the parent
     commit; default this tree), three runs each; the allowance is the baseline's own run-to-run spread. The npz files come from one untimed run
     with --save_captions. The T5 folder is written on the spot: a SentencePiece model trained on a generated corpus and seeded weights at
     T5-XXL's shapes, one safetensors shard per layer. --skip_cli leaves this part out.

The weights are seeded: one layer's tensors are drawn once and uploaded (or saved) under each of the 24 layers' names (separate buffers); timing does
not depend on their values.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16 = 2516.6e12    # dense bf16 MFMA peak of one MI355X
HBM_BPS = 8.0e12
STEP_2048_MS = 115.91    # profiles/dists.txt: the 2048 x 2048 network step
XXL = dict(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=24, vocab_size=32128)


def seeded_layer(cfg):
    """The state dict of a ONE-layer T5 v1.1 encoder at cfg's widths, seeded (transformers' key names)."""
    g = torch.Generator().manual_seed(7)
    D, HD, F = cfg["d_model"], cfg["num_heads"] * cfg["d_kv"], cfg["d_ff"]
    p = "encoder.block.0.layer."
    sd = {"shared.weight": torch.randn(cfg["vocab_size"], D, generator=g), "encoder.final_layer_norm.weight": torch.ones(D),
          p + "0.SelfAttention.relative_attention_bias.weight": torch.randn(32, cfg["num_heads"], generator=g) * 0.5,
          p + "0.layer_norm.weight": torch.ones(D), p + "1.layer_norm.weight": torch.ones(D)}
    for n in ("q", "k", "v"):
        sd[p + f"0.SelfAttention.{n}.weight"] = torch.randn(HD, D, generator=g) * (D ** -0.5 if n != "q" else D ** -0.5 / 8)
    sd[p + "0.SelfAttention.o.weight"] = torch.randn(D, HD, generator=g) * HD ** -0.5
    sd[p + "1.DenseReluDense.wi_0.weight"] = torch.randn(F, D, generator=g) * D ** -0.5
    sd[p + "1.DenseReluDense.wi_1.weight"] = torch.randn(F, D, generator=g) * D ** -0.5
    sd[p + "1.DenseReluDense.wo.weight"] = torch.randn(D, F, generator=g) * F ** -0.5
    return sd


def seeded_xxl(device, layers):
    """models.T5EncoderModel at T5-XXL's shapes with seeded weights on the device (one layer's values under every layer's name): the packed
    tensors are uploaded and bound here, as T5EncoderModel._upload() does for a state dict of all layers, without holding 24 copies on the host."""
    from instarevive_amd import weights as W
    from instarevive_amd.models import T5EncoderModel, get_context
    cfg = dict(XXL, num_layers=layers)
    D, F = cfg["d_model"], cfg["d_ff"]
    sd = seeded_layer(cfg)
    one = W.pack_t5(sd, dict(cfg, num_layers=1))
    enc = T5EncoderModel(**{k: v for k, v in cfg.items()})
    enc.ctx = get_context(device)
    enc.device = enc.ctx.device
    if enc.ctx.lib.ir_drop_optional(enc.ctx.h, b"t5") < 0:
        raise RuntimeError("ir_drop_optional(t5)")
    for k, v in one.items():
        if k.startswith("t5.l0."):
            for i in range(layers):
                enc.ctx.upload(f"t5.l{i}." + k[len("t5.l0."):], v)
        else:
            enc.ctx.upload(k, v)
    enc.ctx.check(enc.ctx.lib.ir_t5_configure(enc.ctx.h, layers, D, cfg["num_heads"], cfg["d_kv"], F, cfg["vocab_size"]), "ir_t5_configure")
    enc._sd = {k: v for k, v in sd.items() if "relative_attention_bias" in k}   # what ensure_bias() reads
    enc._bias_lengths = set()
    enc._mark_bound()
    return enc


def write_t5_folder(d, layers, words):
    """A folder `--t5 DIR` takes, at T5-XXL's shapes: spiece.model trained on `words`, config.json, one bf16 safetensors shard per layer behind an
    index (the layers hold the same seeded values)."""
    import sentencepiece as spm
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    corpus = os.path.join(d, "corpus.txt")
    with open(corpus, "w") as f:
        f.write("\n".join(words))
    spm.SentencePieceTrainer.train(input=corpus, model_prefix=os.path.join(d, "spiece"), vocab_size=200, model_type="unigram", pad_id=0, eos_id=1, unk_id=2,
                                   bos_id=-1, hard_vocab_limit=False, minloglevel=2)
    os.remove(corpus)
    cfg = dict(XXL, num_layers=layers)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(cfg, feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6, relative_attention_num_buckets=32, relative_attention_max_distance=128,
                       model_type="t5"), f)
    sd = {k: v.to(torch.bfloat16).contiguous() for k, v in seeded_layer(cfg).items()}
    shared = {k: v for k, v in sd.items() if not k.startswith("encoder.block.0.") or "relative_attention_bias" in k}
    layer = {k: v for k, v in sd.items() if k not in shared}
    weight_map = {}
    save_file(shared, os.path.join(d, "model-shared.safetensors"))
    weight_map.update({k: "model-shared.safetensors" for k in shared})
    for i in range(layers):
        name = f"model-layer{i:02d}.safetensors"
        part = {k.replace("encoder.block.0.", f"encoder.block.{i}."): v for k, v in layer.items()}
        save_file(part, os.path.join(d, name))
        weight_map.update({k: name for k in part})
    with open(os.path.join(d, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)
    return d


WORDS = ("photo portrait landscape street city forest river mountain face cat dog garden window light shadow detail sharp focus film grain colour "
         "realistic natural skin texture high quality professional evening morning winter summer old new small large red blue green quiet busy").split()


def caption_of(i):
    """A caption of its own for file i, 12 to 20 words from WORDS."""
    rng = np.random.default_rng(1000 + i)
    return "a " + " ".join(rng.choice(WORDS, size=int(rng.integers(12, 21))).tolist()) + f", number {i}"


def cli_leg(a, sds, say):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_text_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        names = sorted(os.listdir(os.path.join(d, "in")))
        caps = {n: caption_of(i) for i, n in enumerate(names)}
        with open(os.path.join(d, "caps.json"), "w") as f:
            json.dump(caps, f)
        t0 = time.perf_counter()
        t5 = write_t5_folder(os.path.join(d, "t5"), a.layers, [" ".join(WORDS)] + list(caps.values()))
        say(f"command line: T5 folder at T5-XXL's shapes ({a.layers} layers, bf16 shards) written in {time.perf_counter() - t0:.1f} s; {a.files} files of 512 x 512, "
            f"--sr_scale 4, one caption of its own per file, T = 300")
        common = ["--input", os.path.join(d, "in"), "--sr_scale", "4", "--png_encoder", "gpu", "--resize", "gpu"] + flags
        text = ["--captions", os.path.join(d, "caps.json"), "--t5", t5]
        npz = os.path.join(d, "npz")
        for how in ("save", "base", "base", "base", "text", "text", "text"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            extra = ["--caption_dir", npz] if how == "base" else text + (["--save_captions", npz] if how == "save" else [])
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(root, "inference.py"), "--output", out] + common + extra, capture_output=True, text=True, timeout=1500,
                               cwd=root)
            wall = time.perf_counter() - t0
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                if how == "save":
                    return
                continue
            if how == "save":
                say(f"untimed run with --save_captions: {len(os.listdir(npz))} npz files, child wall {wall:.1f} s (start-up loads and packs the encoder)")
                continue
            c = rate[0]
            say(f"{'--captions   ' if how == 'text' else '--caption_dir'} ({'this tree' if root == ROOT else 'the parent commit, built'}): {c['files_per_s']:.2f} files/s overall, "
                f"{c['steady_files_per_s']:.2f} after the first result, results left the GPU at {c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host "
                f"threads; child wall {wall:.1f} s, model loading included)")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("text"):
        base, mine = rates["base"], rates["text"]
        spread = max(base) - min(base)
        say(f"--captions {[round(v, 3) for v in mine]} files/s, --caption_dir (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is {spread:.3f} files/s "
            f"({100 * spread / statistics.median(base):.1f} %); median with --captions {statistics.median(mine):.3f} against {statistics.median(base):.3f} "
            f"({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %)")


def timed(fn, warmup, repeats):
    """(median device ms, median host ms of the call itself, all device ms)."""
    dev, host = [], []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn(it)
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            dev.append(e0.elapsed_time(e1))
            host.append(1e3 * (t1 - t0))
    return statistics.median(dev), statistics.median(host), dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=300)
    ap.add_argument("--layers", type=int, default=XXL["num_layers"])
    ap.add_argument("--no_step", action="store_true", help="skip timing the 512 x 512 batch-of-four step (it loads bench.py's full-size models)")
    ap.add_argument("--files", type=int, default=16, help="files of the command line runs")
    ap.add_argument("--skip_cli", action="store_true", help="leave the command line's files/s out")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the --caption_dir runs (default: this tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_prompts.txt"))
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    from instarevive_amd import _lib as L
    from instarevive_amd import text_prompts as TP
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    device = torch.device("cuda", 0)
    T, D = a.tokens, XXL["d_model"]
    enc = seeded_xxl(device, a.layers)
    say(f"T5 encoder at T5-XXL's shapes, {a.layers} layers, seeded weights: {enc.resident_bytes() / 1e9:.2f} GB resident; T = {T}")
    g = torch.Generator().manual_seed(3)
    step4 = sds = None
    results = {}
    for b in (1, 4):
        be = TP.DeviceBackend(enc, T, 8, b)
        ids = [torch.randint(2, XXL["vocab_size"], (b, T), generator=g).to(device, torch.int32) for _ in range(3)]
        mask = torch.zeros(b, T)
        for j in range(b):
            mask[j, :20 + 60 * j] = 1
        dm = mask.to(device)
        flop = 2.0 * b * T * a.layers * (3 * D * D + D * D + 2 * D * XXL["d_ff"] + XXL["d_ff"] * D)
        med, host, ms = timed(lambda it: enc.encode_prompts(ids[it % 3], dm, be.out[:b]), a.warmup, a.repeats)
        floor = 1e3 * flop / PEAK_BF16
        say(f"ir_t5_encode_prompts b = {b}: median {med:.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} calls, 3 rotating id sets); "
            f"{flop / 1e12:.2f} TFLOP in the linears, {100 * floor / med:.1f} % of the {floor:.3f} ms bf16-MFMA floor; the call itself returns after {host:.3f} ms "
            f"on the host ({100 * host / med:.1f} % of the device time: it does not wait)")
        results[b] = med
        lib, ctx = enc.ctx.lib, enc.ctx
        st, _, sms = timed(lambda it: ctx.check(lib.ir_prompt_cache_store(ctx.h, ctx.stream(), L.ptr(be.out[:b]), L.ptr(dm), L.ptr(be.cache), L.ptr(be.cache_mask), 1,
                                                                          be.capacity, (it * b) % (8 - b + 1), b, T, D), "store"), a.warmup, a.repeats)
        byts = b * T * D * 6.0
        say(f"ir_prompt_cache_store b = {b} (fp16): median {1e3 * st:.1f} us (min {1e3 * min(sms):.1f}); {byts / 1e6:.1f} MB moved, {byts / (st * 1e-3) / 1e12:.2f} TB/s = "
            f"{100 * byts / (st * 1e-3) / HBM_BPS:.0f} % of the 8 TB/s HBM peak")
        be.set_fixed(torch.zeros(T, D), torch.ones(T))
        slots = [[(it + j) % 8 if j != 1 else -1 for j in range(b)] for it in range(3)] if b > 1 else [[0], [1], [2]]
        ds = [torch.tensor(s, dtype=torch.int32, device=device) for s in slots]
        y, bias = torch.empty(b, T, D, device=device), torch.empty(b, T, device=device)
        gt, _, gms = timed(lambda it: ctx.check(lib.ir_prompt_gather(ctx.h, ctx.stream(), L.ptr(be.cache), L.ptr(be.cache_mask), 1, be.capacity, L.ptr(ds[it % 3]),
                                                                     L.ptr(be.fixed[0]), L.ptr(be.fixed[1]), L.ptr(y), L.ptr(bias), b, T, D), "gather"), a.warmup, a.repeats)
        say(f"ir_prompt_gather n = {b}: median {1e3 * gt:.1f} us (min {1e3 * min(gms):.1f}); {byts / 1e6:.1f} MB moved, {byts / (gt * 1e-3) / 1e12:.2f} TB/s = "
            f"{100 * byts / (gt * 1e-3) / HBM_BPS:.0f} % of the 8 TB/s HBM peak")
        results[("gather", b)] = gt
        del be
    say(f"share of the recorded 2048 x 2048 step ({STEP_2048_MS} ms, one image, one fresh caption): encode b = 1 {100 * results[1] / STEP_2048_MS:.1f} %, "
        f"gather {100 * results[('gather', 1)] / STEP_2048_MS:.3f} %; a cached caption costs the gather alone")
    if not a.no_step:
        import bench
        from instarevive_amd.pipeline import process
        swin, vae, dit, _sched, sds = bench.build_models(device, lambda m: None)
        yy, mm = bench.synthetic_prompt()
        yy, mm = yy.to(device), mm.to(device)
        rng = np.random.default_rng(1)
        imgs = [rng.integers(0, 255, (512, 512, 3), dtype=np.uint8) for _ in range(4)]
        ts = []
        for it in range(2 + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            process(dit, imgs, 1, "none", False, False, 512, 448, preprocess_model=swin, vae=vae, y=yy, y_mask=mm)
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(1e3 * (time.perf_counter() - t0))
        step4 = statistics.median(ts)
        say(f"512 x 512 batch-of-four step (process() on bench.py's seeded full-size models, wall clock with the host's pre- and post-processing): median "
            f"{step4:.2f} ms (min {min(ts):.2f}, max {max(ts):.2f}, 5 calls)")
        say(f"share of that step: four fresh captions (encode b = 4) {100 * results[4] / step4:.1f} %, gather n = 4 {100 * results[('gather', 4)] / step4:.3f} %; "
            f"captions that are cached cost the gather alone")
    else:
        say("512 x 512 batch-of-four step: not measured in this run (--no_step)")
    say(f"status word after the run: {enc.status()}")
    if a.skip_cli:
        say("command line: not measured in this run (--skip_cli)")
    else:
        enc.release()   # the children load their own encoder
        cli_leg(a, sds, say)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
