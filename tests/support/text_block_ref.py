"""float64 restatement of the two text encoders a part at a time, for the block-level tests of ir_op_text_block
(tests/test_text_block_ref_cpu.py, tests/test_text_block_gpu.py). Four parts, as csrc/api.cpp splits t5_run() / clip_text_run():

    embed(W, ids)                        ids [B][T] -> x [B * T][D]: the embedding rows; CLIP adds positional_embedding[row % T]
    attn(W, layer, x, B, T, key_mask)    the stream behind the attention residual; also the q|k|v rows and the attention output in front of o
    ffn(W, layer, x)                     the stream behind the feed-forward residual
    final(W, x)                          T5: final RMSNorm; CLIP: ln_final

Written from the definitions: transformers' T5Block (T5LayerNorm = x * rsqrt(mean(x^2) + 1e-6) * w with no mean subtracted and no bias;
attention WITHOUT 1 / sqrt(d_kv), with the relative-position bias of block 0 shared by all blocks; wo(gelu_new(wi_0 x) * wi_1 x)) and open_clip's
ResidualAttentionBlock (x + attn(ln_1 x) under the causal mask, q scaled by d_head^-0.5; x + c_proj(gelu(c_fc(ln_2 x))), erf GELU, eps 1e-5).
Everything runs in the dtype and on the device of its inputs.

The bucket of a relative position (`bucket`) is written from the T5 paper's rule in exact integer arithmetic, not from weights.py / oracle/t5.py:
half of the buckets per sign; in a half, distances below half of it are their own bucket, the rest are spaced logarithmically up to max_distance
and everything at or beyond it shares the last one.

The rule for an item whose keys are ALL masked is stated explicitly (`attention`): its rows attend uniformly to all T keys. That is what
transformers computes (finfo.min absorbs score and bias alike), and it is finite.

emulate=True rounds to bf16 where the HIP path stores bf16: xn, q|k|v, the attention output, ab (T5), hid, the weights (CLIP's q rows after the
d_head^-0.5 fold) and the embedding table; the CLIP position add and the final norms run in fp32 there (`fp32=True`: the fp32 yardstick).
mutation=<name> plants one bug (PLANT says where and on which case it is judged).

GATES[key] = (relative L2, worst element / max |reference|), derived in tests/test_text_block_ref_cpu.py and recorded here; none comes from what
the library's kernels measure:
    *_attn, *_ffn (the part's output), *_attn_upd, *_ffn_upd (output - input stream: the residual hides the branch), *_chain: 2 x the emulation's
    error, the largest over the cases of CASES, rounded up to one digit; *_att: the same for the attention output against a float64 softmax over the
    SAME bf16 q|k|v rows (the emulation is then the bf16 rounding of the output alone)
    *_final, clip_embed: 8 x the deviation of the same part evaluated in float32 (an fp32 chain in another summation order: the project's
    convention for those); t5_embed is exact (a bf16 row widened to fp32): (0, 0)
Cases whose own emulation is larger than the common one (OWN_GATES: peaky logits; three narrow CLIP layers chained) carry their own gates in
CASE_GATES, derived the same way from their own emulation, and are left out of the common maximum.
Measured figures: docs/parity.md, section "Text encoders"."""
import math
import zlib

import torch
import torch.nn.functional as F

from tests.golden._det import det_state_dict

T5, CLIP = 0, 1                          # ir_op_text_block encoders
EMBED, ATTN, FFN, FINAL = range(4)       # ir_op_text_block parts
REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
NB, MAXD = 32, 128

# name: (encoder, oracle configuration, q gain)
MODELS = {
    "narrow64": (T5, dict(d_model=256, d_kv=64, num_heads=4, d_ff=512, num_layers=2, vocab_size=300), 1.0),
    "narrow32": (T5, dict(d_model=256, d_kv=32, num_heads=8, d_ff=512, num_layers=2, vocab_size=300), 1.0),
    "peaky64": (T5, dict(d_model=256, d_kv=64, num_heads=4, d_ff=512, num_layers=2, vocab_size=300), 6.8),   # median logit spread about 30 (CPU test)
    "tiny128": (T5, dict(d_model=128, d_kv=32, num_heads=4, d_ff=256, num_layers=1, vocab_size=100), 1.0),   # FINAL at D = 128
    "xxl1": (T5, dict(d_model=4096, d_kv=64, num_heads=64, d_ff=10240, num_layers=1, vocab_size=64), 1.0),
    "clip2": (CLIP, dict(width=128, heads=2, layers=3, vocab_size=300, context_length=77, mlp_ratio=4.0, layer="last"), 1.0),
    "clip4": (CLIP, dict(width=128, heads=4, layers=3, vocab_size=300, context_length=77, mlp_ratio=4.0, layer="last"), 1.0),
    "vith1": (CLIP, dict(width=1024, heads=16, layers=1, vocab_size=300, context_length=77, mlp_ratio=4.0, layer="last"), 1.0),
}
SEEDS = {"narrow64": 2101, "narrow32": 2102, "peaky64": 2101, "tiny128": 2104, "xxl1": 2105, "clip2": 2201, "clip4": 2202, "vith1": 2203}

# planted bug -> (part, the case it is judged on)
PLANT = {
    "scaled_scores": ("attn", "t5_t40x2"), "bias_transposed": ("attn", "t5_t40x2"), "bias_next_head": ("attn", "t5_t40x2"),
    "far_bucket": ("attn", "t5_t300x2"), "log_base": ("attn", "t5_t300x2"), "mask_other_item": ("attn", "t5_t40x2"),
    "mask_on_queries": ("attn", "t5_t40x2"), "full_mask_zeros": ("attn", "t5_fullmask"),
    "rms_mean_subtracted": ("attn", "t5_t40x2"), "gate_halves_swapped": ("ffn", "t5_ffn_77"), "residual_from_norm": ("ffn", "t5_ffn_77"),
    "non_causal": ("attn", "clip2_attn"), "strict_lower": ("attn", "clip2_attn"), "no_q_scale": ("attn", "clip2_attn"),
    "pos_row_bt": ("embed", "clip4_embed"), "post_ln": ("attn", "clip2_attn"), "eps_1e-6": ("attn", "clip2_attn_faint"),
    "gelu_tanh": ("ffn", "clip2_ffn"),
}
MUTATIONS = tuple(PLANT)


def rb(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


# ------------------------------------------------------------------------------------------------ weights
class TextWeights:
    """One encoder as the oracle's state dict `sd` (fp32 tensors; matrices and the embedding table hold bf16 values) and its configuration."""

    def __init__(self, name):
        self.name = name
        self.which, self.cfg, self.q_gain = MODELS[name]
        c = self.cfg
        if self.which == T5:
            from oracle import t5 as o
            self.cfg = dict(o.DEFAULT_CFG, **c)
            self.D, self.H, self.dk, self.F, self.L, self.vocab = c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["num_layers"], c["vocab_size"]
            sd = det_state_dict(o.state_dict_shapes(c), seed=SEEDS[name])
            sd["shared.weight"] = sd["shared.weight"] * math.sqrt(self.D)          # U(+-sqrt 3): rows of unit variance, as a trained table's scale
            sd[REL] = sd[REL] * (3.0 / math.sqrt(3.0 / self.H))                     # U(+-3): bias steps of the order of the scores
            for k in sd:   # T5 folds 1 / sqrt(d_kv) into q's initialisation
                if k.endswith("SelfAttention.q.weight"):
                    sd[k] = sd[k] * (self.dk ** -0.5 * self.q_gain)
        else:
            from oracle import clip_text as o
            self.cfg = dict(o.DEFAULT_CFG, **c)
            self.D, self.H, self.L, self.vocab, self.T = c["width"], c["heads"], c["layers"], c["vocab_size"], c["context_length"]
            self.dk, self.F = self.D // self.H, int(self.D * c["mlp_ratio"])
            sd = det_state_dict(o.state_dict_shapes(c), seed=SEEDS[name])
            sd["token_embedding.weight"] = sd["token_embedding.weight"] * 3.0
            for k in sd:   # q and k of the order that gives attention rows a spread of a few units
                if k.endswith("attn.in_proj_weight"):
                    sd[k] = torch.cat([sd[k][:2 * self.D] * 2.0, sd[k][2 * self.D:]])
        self.sd = {k: (rb(v.float()) if v.dim() == 2 and k != "positional_embedding" else v.float()) for k, v in sd.items()}
        self._dev = {}

    def w(self, name, like):
        """Tensor `name` in the dtype and on the device of `like` (cached)."""
        key = (name, like.device, like.dtype)
        if key not in self._dev:
            self._dev[key] = self.sd[name].to(like.device, like.dtype)
        return self._dev[key]

    def sd64(self):
        return {k: v.double() for k, v in self.sd.items()}


_W = {}


def weights(name):
    if name not in _W:
        _W[name] = TextWeights(name)
    return _W[name]


def drop_weights(name):
    """Forget a model (the full-width ones are large)."""
    _W.pop(name, None)


def model(W):
    """The production model on the GPU with W's weights."""
    if W.which == T5:
        from instarevive_amd.models import T5EncoderModel
        m = T5EncoderModel(**{k: W.cfg[k] for k in ("d_model", "d_kv", "num_heads", "d_ff", "num_layers", "vocab_size")})
    else:
        from instarevive_amd.cldm import FrozenOpenCLIPEmbedder
        c = W.cfg
        m = FrozenOpenCLIPEmbedder(max_length=c["context_length"], layer=c["layer"], width=c["width"], heads=c["heads"], layers=c["layers"],
                                   vocab_size=c["vocab_size"], mlp_ratio=c["mlp_ratio"])
    m.load_state_dict(W.sd, strict=True)
    return m.to("cuda")


# ------------------------------------------------------------------------------------------------ relative-position buckets (T5 paper, section 2.1)
def bucket(rel, num_buckets=NB, max_distance=MAXD, mutation=None):
    """Bucket of rel = key position - query position, bidirectional. Exact integers: with h = num_buckets / 2 buckets per sign and e = h / 2 exact
    ones, a distance n >= e falls into e + floor((h - e) * log(n / e) / log(max_distance / e)), capped at h - 1; the floor is the largest k with
    (max_distance / e)^k <= (n / e)^(h - e), i.e. max_distance^k * e^(h - e) <= n^(h - e) * e^k."""
    h = num_buckets // 2
    e = h // 2
    n = abs(int(rel))
    if mutation == "log_base":
        max_distance = 2 * max_distance
    if n < e:
        b = n
    else:
        k = 0
        while k + 1 <= h and max_distance ** (k + 1) * e ** (h - e) <= n ** (h - e) * e ** (k + 1):
            k += 1
        cap = h - 2 if mutation == "far_bucket" and n >= max_distance else h - 1
        b = min(e + k, cap)
    return b + (h if rel > 0 else 0)


def bucket_table(lo=-511, hi=511, mutation=None):
    """[hi - lo + 1] int64: bucket(rel) for rel = lo .. hi."""
    return torch.tensor([bucket(r, mutation=mutation) for r in range(lo, hi + 1)], dtype=torch.int64)


def t5_bias(W, T, like, mutation=None):
    """The additive bias [H][T][T] (query, key) of a T5 model at T tokens."""
    tab = bucket_table(-(T - 1), T - 1, mutation if mutation in ("far_bucket", "log_base") else None) if T > 1 else torch.tensor([bucket(0)])
    pos = torch.arange(T)
    idx = tab[(pos[None, :] - pos[:, None]) + (T - 1)].to(like.device)   # [q][k]
    b = W.w(REL, like)[idx].permute(2, 0, 1)
    if mutation == "bias_transposed":
        b = b.transpose(1, 2)
    if mutation == "bias_next_head":
        b = b.roll(-1, 0)
    return b.contiguous()


# ------------------------------------------------------------------------------------------------ the parts
def attention(q, k, v, bias, key_mask=None, mutation=None):
    """q, k, v [B][H][T][dk], bias [H][T][T] (may hold -inf), key_mask [B][T] (1 = token) or None -> [B][H][T][dk]. A masked key has weight 0;
    an item whose keys are ALL masked attends uniformly to all T keys."""
    s = q @ k.transpose(-1, -2) + bias
    none = None
    if key_mask is not None and mutation != "mask_on_queries":
        dead = (key_mask < 0.5)[:, None, None, :]
        none = dead.all(-1, keepdim=True)
        s = torch.where(none, torch.zeros_like(s), s.masked_fill(dead, float("-inf")))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)   # (only a planted bug makes an empty row)
    if none is not None and mutation == "full_mask_zeros":
        p = torch.where(none, torch.zeros_like(p), p)
    if key_mask is not None and mutation == "mask_on_queries":
        p = p * (key_mask >= 0.5).to(p.dtype)[:, None, :, None]
    return p @ v


def split_heads(qkv, B, T, H, dk):
    """[B * T][3 * H * dk] -> q, k, v [B][H][T][dk]."""
    return (t.reshape(B, T, H, dk).transpose(1, 2) for t in qkv.chunk(3, dim=-1))


def causal(T, like, mutation=None):
    if mutation == "non_causal":
        return torch.zeros(T, T, dtype=like.dtype, device=like.device)
    return torch.full((T, T), float("-inf"), dtype=like.dtype, device=like.device).triu_(0 if mutation == "strict_lower" else 1)


def att_from_qkv(W, qkv, B, T, key_mask=None):
    """The attention output [B * T][H * dk] in the dtype of qkv from GIVEN q|k|v rows (the kernel's own bf16 ones, widened)."""
    q, k, v = split_heads(qkv, B, T, W.H, W.dk)
    bias = t5_bias(W, T, qkv) if W.which == T5 else causal(T, qkv)
    return attention(q, k, v, bias, key_mask).transpose(1, 2).reshape(B * T, W.H * W.dk)


def rmsnorm(x, w, eps=1e-6, mutation=None):
    if mutation == "rms_mean_subtracted":
        x = x - x.mean(-1, keepdim=True)
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def embed(W, ids, emulate=False, mutation=None):
    """ids [B][T] (long) -> x [B * T][D] (float64; the CLIP position add in fp32 under emulate)."""
    B, T = ids.shape
    like = torch.zeros((), dtype=torch.float64, device=ids.device)
    if W.which == T5:
        return W.w("shared.weight", like)[ids.reshape(-1)]
    x = W.w("token_embedding.weight", like)[ids.reshape(-1)]
    pos = W.w("positional_embedding", like)
    rows = torch.arange(B * T, device=ids.device)
    if mutation == "pos_row_bt":   # row % (B * T): behind the first item the table has no rows
        pos = torch.cat([pos, torch.zeros((B - 1) * T, W.D, dtype=pos.dtype, device=pos.device)])
        add = pos[rows % (B * T)]
    else:
        add = pos[rows % T]
    return (x.float() + add.float()).double() if emulate else x + add


def attn(W, layer, x, B, T, key_mask=None, emulate=False, mutation=None):
    """-> dict(x: the stream behind the attention residual, qkv: the rows the attention read, att: its output in front of the o-projection)."""
    r = rb if emulate else (lambda t: t)
    H, dk, D = W.H, W.dk, W.D
    if W.which == T5:
        p = f"encoder.block.{layer}.layer.0."
        xn = r(rmsnorm(x, W.w(p + "layer_norm.weight", x), mutation=mutation))
        wq = torch.cat([W.w(p + f"SelfAttention.{n}.weight", x) for n in ("q", "k", "v")], 0)
        qkv = r(xn @ wq.t())
        q, k, v = split_heads(qkv, B, T, H, dk)
        if mutation == "scaled_scores":
            q = q * dk ** -0.5
        km = key_mask.roll(1, 0) if mutation == "mask_other_item" else key_mask
        a = attention(q, k, v, t5_bias(W, T, x, mutation), km, mutation)
        att = r(a.transpose(1, 2).reshape(B * T, H * dk))
        return dict(x=x + att @ W.w(p + "SelfAttention.o.weight", x).t(), qkv=qkv, att=att)
    p = f"transformer.resblocks.{layer}."
    eps = 1e-6 if mutation == "eps_1e-6" else 1e-5
    xn = r(F.layer_norm(x, (D,), W.w(p + "ln_1.weight", x), W.w(p + "ln_1.bias", x), eps))
    scale = 1.0 if mutation == "no_q_scale" else dk ** -0.5
    wq, bq = W.w(p + "attn.in_proj_weight", x).clone(), W.w(p + "attn.in_proj_bias", x).clone()
    wq[:D] *= scale      # the production path folds the scale into the q rows and stores THEM as bf16
    bq[:D] *= scale
    if emulate:
        wq, bq = rb(wq), bq.float().to(x.dtype)
    qkv = r(xn @ wq.t() + bq)
    q, k, v = split_heads(qkv, B, T, H, dk)
    att = r(attention(q, k, v, causal(T, x, mutation)).transpose(1, 2).reshape(B * T, D))
    y = x + att @ W.w(p + "attn.out_proj.weight", x).t() + W.w(p + "attn.out_proj.bias", x)
    if mutation == "post_ln":
        y = F.layer_norm(y, (D,), W.w(p + "ln_1.weight", x), W.w(p + "ln_1.bias", x), eps)
    return dict(x=y, qkv=qkv, att=att)


def ffn(W, layer, x, emulate=False, mutation=None):
    """-> the stream behind the feed-forward residual."""
    r = rb if emulate else (lambda t: t)
    if W.which == T5:
        p = f"encoder.block.{layer}.layer.1."
        xn = r(rmsnorm(x, W.w(p + "layer_norm.weight", x)))
        a, b = r(xn @ W.w(p + "DenseReluDense.wi_0.weight", x).t()), r(xn @ W.w(p + "DenseReluDense.wi_1.weight", x).t())
        if mutation == "gate_halves_swapped":
            a, b = b, a
        hid = r(gelu_new(a) * b)
        return (xn if mutation == "residual_from_norm" else x) + hid @ W.w(p + "DenseReluDense.wo.weight", x).t()
    p = f"transformer.resblocks.{layer}."
    xn = r(F.layer_norm(x, (W.D,), W.w(p + "ln_2.weight", x), W.w(p + "ln_2.bias", x), 1e-5))
    h = xn @ W.w(p + "mlp.c_fc.weight", x).t() + W.w(p + "mlp.c_fc.bias", x)
    hid = r(gelu_new(h) if mutation == "gelu_tanh" else F.gelu(h))
    return x + hid @ W.w(p + "mlp.c_proj.weight", x).t() + W.w(p + "mlp.c_proj.bias", x)


def final(W, x, fp32=False):
    """T5: the final RMSNorm; CLIP: ln_final. fp32: the same evaluated in float32 (the yardstick of its gate)."""
    xx = x.float() if fp32 else x
    if W.which == T5:
        y = rmsnorm(xx, W.w("encoder.final_layer_norm.weight", xx))
    else:
        y = F.layer_norm(xx, (W.D,), W.w("ln_final.weight", xx), W.w("ln_final.bias", xx), 1e-5)
    return y.to(x.dtype)


def chain(W, ids, key_mask=None, emulate=False):
    """EMBED -> (ATTN, FFN) x L -> FINAL."""
    B, T = ids.shape
    x = embed(W, ids, emulate)
    for l in range(W.L):
        x = attn(W, l, x, B, T, key_mask, emulate)["x"]
        x = ffn(W, l, x, emulate)
    return final(W, x, fp32=emulate)


# ------------------------------------------------------------------------------------------------ inputs, errors
def make_stream(rows, D, seed, kind=""):
    """fp32 rows [rows][D] ~ N(0, 1) + a per-channel offset of std 0.5; "outlier": 1 % of the channels x 100; "faint": everything x 2e-3."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g, dtype=torch.float64) + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)
    if kind == "outlier":
        ch = torch.randperm(D, generator=g)[:max(1, D // 100)]
        x[:, ch] *= 100.0
    if kind == "faint":
        x *= 2e-3
    return x.float()


def make_ids(B, T, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 1, (B, T), generator=g)
    ids[0, 0], ids[-1, -1] = 0, vocab - 1   # the first and the last row of the table
    return ids


def make_mask(B, T, valid):
    """valid: None (no mask), a tuple of valid lengths, or ("hole", a, b): everything valid but keys a .. b - 1."""
    if valid is None:
        return None
    m = torch.zeros(B, T)
    if valid[0] == "hole":
        m[:] = 1
        m[:, valid[1]:valid[2]] = 0
        return m
    for i, n in enumerate(valid):
        m[i, :n] = 1
    return m


def errors(got, ref):
    """(relative L2, worst element / max |ref|)."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


def outside(e, gate):
    """The largest measured / gate ratio over the two metrics."""
    return max(e[0] / gate[0], e[1] / gate[1])


def round_up(v):
    """v rounded up to one significant digit."""
    if v <= 0:
        return 0.0
    p = 10.0 ** math.floor(math.log10(v))
    return float(f"{math.ceil(v / p - 1e-9) * p:.0e}")


def logit_spread(W, x, B, T, key_mask=None):
    """Median over rows of max - min of the scores over the row's valid keys (layer 0)."""
    q, k, _ = split_heads(attn(W, 0, x, B, T, key_mask)["qkv"], B, T, W.H, W.dk)
    s = q @ k.transpose(-1, -2) + t5_bias(W, T, x)
    if key_mask is not None:
        dead = (key_mask < 0.5)[:, None, None, :].expand_as(s)
        hi, lo = s.masked_fill(dead, float("-inf")).amax(-1), s.masked_fill(dead, float("inf")).amin(-1)
    else:
        hi, lo = s.amax(-1), s.amin(-1)
    return float((hi - lo).median())


# ------------------------------------------------------------------------------------------------ cases (shared by the CPU and the GPU test)
# id: (part, model, layer, B, T, mask, stream: "" / "outlier" (1 % of the channels x 100) / "faint" (x 2e-3: the norm's eps carries weight)).  T5 ATTN: 1 token; two items of different lengths; one query tile exactly and one row more;
# 120 (the product's length); 300: distances >= 128 act on valid keys and the kernel's LDS passes 64 KiB; 512: all eight keys per lane, dk 64 and 32;
# a hole in the mask; no mask; an item with every key masked between two that are not; peaky logits; outlier channels; the full width
CASES = {
    "t5_t1": ("attn", "narrow64", 0, 1, 1, (1,), ""), "t5_t40x2": ("attn", "narrow64", 1, 2, 40, (40, 7), ""),
    "t5_t64": ("attn", "narrow32", 0, 1, 64, (64,), ""), "t5_t65": ("attn", "narrow64", 0, 1, 65, (65,), ""),
    "t5_t120x2": ("attn", "narrow32", 1, 2, 120, (120, 33), ""), "t5_t300x2": ("attn", "narrow64", 0, 2, 300, (300, 170), ""),
    "t5_t512_dk64": ("attn", "narrow64", 0, 1, 512, (400,), ""), "t5_t512_dk32": ("attn", "narrow32", 0, 1, 512, (400,), ""),
    "t5_t77_hole": ("attn", "narrow64", 0, 1, 77, ("hole", 20, 31), ""), "t5_nomask": ("attn", "narrow32", 0, 2, 40, None, ""),
    "t5_fullmask": ("attn", "narrow64", 0, 3, 24, (24, 0, 11), ""), "t5_peaky": ("attn", "peaky64", 0, 2, 120, (120, 33), ""),
    "t5_outlier": ("attn", "narrow64", 0, 1, 77, (77,), "outlier"), "t5_xxl1": ("attn", "xxl1", 0, 2, 120, (120, 33), ""),
    "t5_ffn_1": ("ffn", "narrow64", 0, 1, 1, None, ""), "t5_ffn_77": ("ffn", "narrow64", 1, 1, 77, None, ""),
    "t5_ffn_240": ("ffn", "narrow32", 0, 2, 120, None, ""), "t5_ffn_600": ("ffn", "narrow64", 0, 2, 300, None, ""),
    "t5_ffn_xxl1": ("ffn", "xxl1", 0, 2, 120, None, ""), "t5_ffn_outlier": ("ffn", "narrow64", 0, 1, 77, None, "outlier"),
    "t5_embed": ("embed", "narrow64", 0, 2, 40, None, ""), "clip4_embed": ("embed", "clip4", 0, 3, 77, None, ""),
    "t5_final_1_d128": ("final", "tiny128", 0, 1, 1, None, ""), "t5_final_5_d128": ("final", "tiny128", 0, 1, 5, None, ""),
    "t5_final_240_d128": ("final", "tiny128", 0, 2, 120, None, ""),
    "t5_final_1_d256": ("final", "narrow64", 0, 1, 1, None, ""), "t5_final_5_d256": ("final", "narrow64", 0, 1, 5, None, ""),
    "t5_final_240_d256": ("final", "narrow64", 0, 2, 120, None, ""),
    "t5_final_1_d4096": ("final", "xxl1", 0, 1, 1, None, ""), "t5_final_5_d4096": ("final", "xxl1", 0, 1, 5, None, ""),
    "t5_final_240_d4096": ("final", "xxl1", 0, 2, 120, None, ""),
    "clip2_final": ("final", "clip2", 0, 1, 77, None, ""), "vith1_final": ("final", "vith1", 0, 2, 77, None, ""),
    "clip2_attn": ("attn", "clip2", 1, 1, 77, None, ""), "clip4_attn": ("attn", "clip4", 2, 3, 77, None, ""),
    "vith1_attn": ("attn", "vith1", 0, 2, 77, None, ""), "clip2_attn_faint": ("attn", "clip2", 0, 1, 77, None, "faint"),
    "clip2_ffn": ("ffn", "clip2", 1, 1, 77, None, ""), "clip4_ffn": ("ffn", "clip4", 2, 3, 77, None, ""),
    "vith1_ffn": ("ffn", "vith1", 0, 2, 77, None, ""),
    "clip2_chain": ("chain", "clip2", 0, 1, 77, None, ""), "clip4_chain": ("chain", "clip4", 0, 3, 77, None, ""),
    "vith1_chain": ("chain", "vith1", 0, 2, 77, None, ""),
    "t5_chain": ("chain", "narrow64", 0, 2, 40, (40, 7), ""), "t5_chain_dk32": ("chain", "narrow32", 0, 3, 24, (24, 0, 11), ""),
}


def case_seed(case):
    return zlib.crc32(case.encode()) % 100000   # (does not move when a case is added)


def case_inputs(case):
    """(ids [B][T] long or None, x fp32 [B * T][D] or None, key_mask fp32 [B][T] or None) on the CPU."""
    part, name, _, B, T, valid, outl = CASES[case]
    W = weights(name)
    mask = make_mask(B, T, valid)
    if part in ("embed", "chain"):
        return make_ids(B, T, W.vocab, case_seed(case)), None, mask
    return None, make_stream(B * T, W.D, case_seed(case), outl), mask


def run_case(case, ins, emulate=False, mutation=None):
    """{gate key suffix: output} of the case's part on `ins` = (ids, x in float64, key_mask), on the device of the inputs."""
    part, name, layer, B, T, _, _ = CASES[case]
    W = weights(name)
    ids, x, mask = ins
    if part == "embed":
        return {"embed": embed(W, ids, emulate, mutation)}
    if part == "attn":
        o = attn(W, layer, x, B, T, mask, emulate, mutation)
        return {"attn": o["x"], "attn_upd": o["x"] - x, "qkv": o["qkv"], "att_raw": o["att"]}
    if part == "ffn":
        y = ffn(W, layer, x, emulate, mutation)
        return {"ffn": y, "ffn_upd": y - x}
    if part == "final":
        return {"final": final(W, x, fp32=emulate)}
    return {"chain": chain(W, ids, mask, emulate)}


GATED = {"embed": ("embed",), "attn": ("attn", "attn_upd"), "ffn": ("ffn", "ffn_upd"), "final": ("final",), "chain": ("chain",)}


def prefix(case):
    return "t5_" if MODELS[CASES[case][1]][0] == T5 else "clip_"


def measure(case, got, ref):
    """{gate key: (rel-L2, worst)} of a case's gated outputs against the reference's."""
    return {prefix(case) + k: errors(got[k], ref[k]) for k in GATED[CASES[case][0]]}


def gates_of(case):
    """{gate key: (rel-L2 gate, worst gate)} of a case (its own where CASE_GATES has them)."""
    keys = [prefix(case) + k for k in GATED[CASES[case][0]]] + ([prefix(case) + "att"] if CASES[case][0] == "attn" else [])
    return {k: CASE_GATES.get(case, {}).get(k, GATES[k]) for k in keys}


MARGIN = 2.0        # emulation -> gate
FP32_MARGIN = 8.0   # fp32 yardstick -> gate
FP32_KEYS = ("t5_final", "clip_final", "clip_embed")
OWN_GATES = ("t5_peaky", "clip2_chain", "clip4_chain")   # cases whose emulation is not the common one: peaky logits; three narrow layers chained
GATES = {
    "t5_embed": (0.0, 0.0), "t5_attn": (3e-3, 5e-3), "t5_attn_upd": (6e-3, 8e-3), "t5_att": (4e-3, 7e-3), "t5_ffn": (5e-3, 5e-3),
    "t5_ffn_upd": (1e-2, 2e-2), "t5_final": (9e-7, 2e-6), "t5_chain": (8e-3, 9e-3),
    "clip_embed": (3e-7, 4e-7), "clip_attn": (7e-3, 2e-2), "clip_attn_upd": (2e-2, 2e-2), "clip_att": (4e-3, 6e-3), "clip_ffn": (3e-3, 3e-3),
    "clip_ffn_upd": (5e-3, 6e-3), "clip_final": (6e-7, 2e-6), "clip_chain": (2e-2, 2e-2),
}
CASE_GATES = {"t5_peaky": {"t5_attn": (9e-3, 2e-2), "t5_attn_upd": (2e-2, 3e-2)}, "clip2_chain": {"clip_chain": (3e-2, 3e-2)},
              "clip4_chain": {"clip_chain": (3e-2, 5e-2)}}
# planted bugs that no bf16 gate can see, with the largest measured / gate ratio they reach on their case (kept in PLANT, asserted as recorded)
INVISIBLE = {"gelu_tanh": 0.04}
