"""Third-party pins of the two text encoders as data: tests/golden/text_pins.npz, written from the installed `transformers` alone (with oracle/ for
the state-dict shapes and tests/golden/_det.py for the seeded weights; the reference tree is not needed). Run: python -m tests.golden.make_text_pins

    (a) bucket        transformers' T5Attention._relative_position_bucket for rel = -511 .. 511 (bidirectional, 32 buckets, max distance 128)
    (b) t5_long_*     T5EncoderModel at T5_SMALL, b = 2, T = 300, valid lengths (300, 170): distances >= 128 act on valid keys
    (c) t5_full_*     the same model at b = 3, T = 24 with item 1 fully masked (its rows are finite: uniform attention over all 24 keys)
    (d) clip_*        CLIPTextModel (hidden_act "gelu", layer_norm_eps 1e-5: an independent port of open_clip's text tower) at width 128, 4 heads,
                      3 layers, vocab 300, T = 77, with the end-of-text id at position 9 in one item and 76 in the other: last_hidden_state
                      ("last") and final_layer_norm(hidden_states[-2]) ("penultimate")
Only the ids, masks, outputs and a weight checksum are stored; tests/test_text_block_ref_cpu.py rebuilds the weights from the seeds below."""
import os

import numpy as np
import torch

from tests.golden._det import checksum, det_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
T5_SMALL = dict(d_model=128, d_kv=32, num_heads=4, d_ff=256, num_layers=2, vocab_size=100)
CLIP_SMALL = dict(width=128, heads=4, layers=3, vocab_size=300, context_length=77, mlp_ratio=4.0)
T5_SEED, CLIP_SEED = 707, 911


def t5_small_sd():
    from oracle import t5 as ot5
    sd = det_state_dict(ot5.state_dict_shapes(T5_SMALL), seed=T5_SEED)
    sd["shared.weight"] = sd["shared.weight"] * 8.0
    for k in sd:   # T5 folds 1 / sqrt(d_kv) into q's initialisation
        if k.endswith("SelfAttention.q.weight"):
            sd[k] = sd[k] * T5_SMALL["d_kv"] ** -0.5
    return sd


def clip_small_sd():
    from oracle import clip_text as oclip
    return det_state_dict(oclip.state_dict_shapes(CLIP_SMALL), seed=CLIP_SEED)


def clip_to_transformers(sd, cfg, names):
    """open_clip text-tower names -> transformers.CLIPTextModel names (`names`: the model's own keys; newer versions have no `text_model.` prefix)."""
    pre = "text_model." if any(k.startswith("text_model.") for k in names) else ""
    d = cfg["width"]
    out = {pre + "embeddings.token_embedding.weight": sd["token_embedding.weight"],
           pre + "embeddings.position_embedding.weight": sd["positional_embedding"],
           pre + "final_layer_norm.weight": sd["ln_final.weight"], pre + "final_layer_norm.bias": sd["ln_final.bias"]}
    for i in range(cfg["layers"]):
        s, t = f"transformer.resblocks.{i}.", pre + f"encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):   # in_proj_* split into q / k / v
            out[t + f"self_attn.{n}.weight"] = sd[s + "attn.in_proj_weight"][j * d:(j + 1) * d]
            out[t + f"self_attn.{n}.bias"] = sd[s + "attn.in_proj_bias"][j * d:(j + 1) * d]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"),
                     ("mlp.c_proj", "mlp.fc2")):
            out[t + b + ".weight"], out[t + b + ".bias"] = sd[s + a + ".weight"], sd[s + a + ".bias"]
    return out


def t5_inputs():
    g = np.random.Generator(np.random.PCG64(78))
    ids_long = torch.from_numpy(g.integers(2, 100, size=(2, 300))).long()
    mask_long = torch.ones(2, 300, dtype=torch.long)
    mask_long[1, 170:] = 0
    ids_full = torch.from_numpy(g.integers(2, 100, size=(3, 24))).long()
    mask_full = torch.ones(3, 24, dtype=torch.long)
    mask_full[1] = 0
    mask_full[2, 11:] = 0
    return ids_long * mask_long, mask_long, ids_full * mask_full, mask_full


def clip_inputs():
    g = np.random.Generator(np.random.PCG64(79))
    v = CLIP_SMALL["vocab_size"]
    ids = torch.from_numpy(g.integers(1, v - 2, size=(2, 77))).long()
    ids[:, 0] = v - 2          # start of text
    ids[0, 9] = v - 1          # end of text (the largest id), then padding
    ids[0, 10:] = 0
    ids[1, 76] = v - 1
    return ids


@torch.no_grad()
def main():
    import transformers
    from transformers.models.t5.modeling_t5 import T5Attention
    rel = torch.arange(-511, 512)
    bucket = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=32, max_distance=128)

    hf = transformers.T5Config(feed_forward_proj="gated-gelu", relative_attention_num_buckets=32, relative_attention_max_distance=128,
                               layer_norm_epsilon=1e-6, dropout_rate=0.0, tie_word_embeddings=False, **T5_SMALL)
    m = transformers.T5EncoderModel(hf).eval()
    sd = t5_small_sd()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("embed_tokens" in k for k in missing), (missing, unexpected)
    ids_long, mask_long, ids_full, mask_full = t5_inputs()
    out_long = m(input_ids=ids_long, attention_mask=mask_long)["last_hidden_state"]
    out_full = m(input_ids=ids_full, attention_mask=mask_full)["last_hidden_state"]
    assert torch.isfinite(out_full).all()

    c = CLIP_SMALL
    cc = transformers.CLIPTextConfig(vocab_size=c["vocab_size"], hidden_size=c["width"], intermediate_size=int(c["width"] * c["mlp_ratio"]),
                                     num_hidden_layers=c["layers"], num_attention_heads=c["heads"], max_position_embeddings=c["context_length"],
                                     hidden_act="gelu", layer_norm_eps=1e-5, attention_dropout=0.0, bos_token_id=c["vocab_size"] - 2,
                                     eos_token_id=c["vocab_size"] - 1, pad_token_id=0)
    cm = transformers.CLIPTextModel(cc).eval()
    csd = clip_small_sd()
    names = list(cm.state_dict())
    missing, unexpected = cm.load_state_dict(clip_to_transformers(csd, c, names), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    ids = clip_inputs()
    o = cm(input_ids=ids, output_hidden_states=True)
    fln = (cm.text_model if hasattr(cm, "text_model") and hasattr(cm.text_model, "final_layer_norm") else cm).final_layer_norm
    last, pen = o.last_hidden_state, fln(o.hidden_states[-2])

    np.savez_compressed(os.path.join(HERE, "text_pins.npz"), bucket=bucket.numpy().astype(np.int16),
                        t5_wsum=checksum(sd), t5_long_ids=ids_long.numpy().astype(np.int16), t5_long_mask=mask_long.numpy().astype(np.uint8),
                        t5_long_out=out_long.numpy(), t5_full_ids=ids_full.numpy().astype(np.int16), t5_full_mask=mask_full.numpy().astype(np.uint8),
                        t5_full_out=out_full.numpy(), clip_wsum=checksum(csd), clip_ids=ids.numpy().astype(np.int16), clip_last=last.numpy(),
                        clip_penultimate=pen.numpy(),
                        note=f"transformers {transformers.__version__}: T5EncoderModel (gated-gelu, 2 blocks of width 128), CLIPTextModel (gelu, 3 layers of width 128)")
    print("wrote text_pins.npz", os.path.getsize(os.path.join(HERE, "text_pins.npz")), "bytes")


if __name__ == "__main__":
    main()
