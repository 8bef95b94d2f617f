#!/usr/bin/env python3
"""Write the per-image caption files inference.py / eval_batch.py consume (--caption_dir) and the reference's datasets read
(dataset/codeformer.py:765-790): `<t5_save_root>/<key without extension>.npz` with `caption_feature` fp16 [1, T, 4096] and `attention_mask`
int16 [1, T], one per entry of a {file name: caption} JSON.

This is the reference's producer (tools/extract_caption.py --run_t5_feature_extract: T5Tokenizer(max_length, padding="max_length", truncation) ->
T5EncoderModel -> np.savez_compressed) on the MI355X path, under its flag names: the tokenizer from a LOCAL folder, the HIP T5 encoder, captions
encoded --batch_size at a time on the device (ir_t5_encode_prompts -> ir_prompt_cache_store: the fp16 rounding of `caption_emb.to(torch.float16)`).

    python tools/make_captions.py --t5_json_path captions.json --t5_models_dir /models/PixArt-XL-2-512x512 --t5_save_root caps --max_length 300

--t5_models_dir holds tokenizer/ and text_encoder/ subfolders, as the reference expects, or the files themselves (DeepFloyd/t5-v1_1-xxl layout).
An existing file is kept, as the reference keeps it. A caption is stripped of surrounding white space (extract_caption.py:150); --clean applies
T5Embedder.text_preprocessing first (the reference's producer feeds the raw caption, which is the default here too)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t5_json_path", required=True, help="{file name: caption}")
    ap.add_argument("--t5_models_dir", required=True, help="folder with tokenizer/ and text_encoder/ subfolders, or with the T5 files themselves")
    ap.add_argument("--t5_save_root", required=True)
    ap.add_argument("--max_length", type=int, default=300)
    ap.add_argument("--batch_size", type=int, default=4, help="captions per encoder call")
    ap.add_argument("--clean", action="store_true", help="apply T5Embedder.text_preprocessing to every caption first")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    if not 1 <= args.max_length <= 512:
        raise SystemExit("--max_length: the T5 encoder takes 1 .. 512 tokens")
    import torch
    from instarevive_amd import text_prompts as TP
    with open(args.t5_json_path, encoding="utf-8") as f:
        table = json.load(f)
    if not isinstance(table, dict) or not all(isinstance(v, str) for v in table.values()):
        raise SystemExit(f"{args.t5_json_path}: a caption JSON is one object {{file name: caption}}")
    where = dict(t5_pipeline=args.t5_models_dir) if os.path.isdir(os.path.join(args.t5_models_dir, "tokenizer")) else dict(t5=args.t5_models_dir)
    tokenizer = TP.load_tokenizer(**where)
    enc = TP.load_encoder(torch.device(args.device), **where)
    bs = max(args.batch_size, 1)
    backend = TP.DeviceBackend(enc, args.max_length, bs, bs)
    print(f"T5 encoder resident: {backend.resident_bytes() / 1e9:.2f} GB; T = {args.max_length}, {bs} captions per call")
    todo = []
    for key, caption in table.items():
        path = os.path.join(args.t5_save_root, os.path.splitext(key)[0] + ".npz")
        if not os.path.exists(path):
            todo.append((path, TP.clean(caption.strip(), args.clean)))
    for i in range(0, len(todo), bs):
        part = todo[i:i + bs]
        ids, mask = TP.tokenize(tokenizer, [c for _, c in part], args.max_length)
        backend.encode_store(ids, mask, list(range(len(part))))
        for j, (path, _) in enumerate(part):
            TP.save_caption(path, *backend.read_slot(j))
    if backend.status():
        raise SystemExit("the encoder reported an id outside its vocabulary: the files of this run are not to be trusted")
    print(f"saved {len(todo)} caption files under {args.t5_save_root} ({len(table) - len(todo)} existed already)")


if __name__ == "__main__":
    main()
