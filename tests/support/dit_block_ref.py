"""float64 restatement of ONE PixArt DiT block (ada_norm_single BasicTransformerBlock: oracle/dit.py's `block` closure) from the token stream on,
with what feeds it: the timestep -> t_block -> scale_shift_table modulation rows, the caption projection of the raw 4096-wide prompt and its
cross-attention K / V, the additive key bias, and item b's prompt slot b % P. Optional qk_norm and KV compression (conv sampler, r = 2).

Weights: tests.golden._det.det_state_dict at full width (1 layer, 16 x 72 heads, mlp 4608, caption 4096), rounded to bf16 - the values the
production path (weights.pack_dit / Transformer2DModel) uploads - with two gains so that the block is not trivially flat: attn1.to_q / to_k
(or, under qk_norm, the q / k norms) scaled so that self-attention logits have a std of about 3, and adaln_single.linear scaled so that each
of the three branches (self-attention, cross-attention, MLP) moves the update visibly (tests/test_dit_block_ref_cpu.py asserts both).

Token rows: [n * T][1152] float64, item-major (T = gh * gw). Every function runs on the device of its inputs, so the GPU test evaluates the
same code in float64 on the GPU; the attention is chunked by query blocks so that T = 16384 fits.

`emulate=True` rounds to bf16 where the HIP path stores bf16: the modulated LN outputs, the qkv rows (after qk_norm / compression), P before PV,
O, the bf16 copy of the stream the cross-attention q is projected from, cq, the GELU hidden units and the prompt path (embeds, caption MLP,
K / V cache). `mutation` plants one bug (MUTATIONS), to show that the gates see it."""
import math

import torch
import torch.nn.functional as F

from oracle import dit as odit
from tests.golden._det import det_state_dict

HEADS, HD, C, MLP, CAP = 16, 72, 1152, 4608, 4096
Q_GAIN = 1.45      # attn1.to_q / to_k (weight and bias): self-attention logit std about 3
MOD_GAIN = 2.0     # adaln_single.linear (weight and bias): gates and scales of order one
PEAKY_GAIN = 3.5   # q / k gain on top of Q_GAIN for peaky scores (logit std about 37): the DiT self-attention's fixed softmax reference overflows
# gates (relative L2, worst element / max |update|) on the block's update. Peaky scores magnify the bf16 rounding of q and k themselves (the CPU
# emulation measures about 1.5e-2 / 3.1e-2 there), so that case is gated from its emulation with 2x margin and leans on the plain-route ratio.
GATES = dict(base=(1e-2, 1e-2), peaky=(4e-2, 8e-2))
KVC = dict(sampling="conv", scale_factor=2, layers=(0,))
MUTATIONS = ("o_heads_swapped", "v_tail_from_next_head", "scale_without_one", "msa_mlp_rows_swapped", "last_token_masked",
             "prompt_slot_shifted", "gate_msa_on_cross", "softmax_scale_1_over_8")
P_ = "transformer_blocks.0."


def rb(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


class DitWeights:
    """One full-width DiT layer: `sd` holds the bf16-rounded tensors under the diffusers names (what Transformer2DModel.load_state_dict takes),
    `cfg` the oracle's configuration of that model."""

    def __init__(self, seed=505, qk_norm=False, kv_compress=False, q_gain=Q_GAIN):
        self.cfg = dict(num_layers=1, qk_norm=qk_norm, kv_compress=dict(KVC) if kv_compress else None)
        sd = det_state_dict(odit.state_dict_shapes(self.cfg), seed=seed)
        for k in list(sd):
            if k.startswith((P_ + "attn1.to_q.", P_ + "attn1.to_k.")) and not qk_norm:
                sd[k] = sd[k] * q_gain
            if k.startswith((P_ + "attn1.q_norm.", P_ + "attn1.k_norm.")):
                sd[k] = sd[k] * 3.0 ** 0.5
            if k.startswith("adaln_single.linear."):
                sd[k] = sd[k] * MOD_GAIN
        self.sd = {k: rb(v) for k, v in sd.items()}
        self.qk_norm, self.kvc = qk_norm, kv_compress
        self._dev = {}

    def w(self, name, like):
        """Tensor `name` in float64 on the device of `like` (cached per device)."""
        key = (name, like.device)
        if key not in self._dev:
            self._dev[key] = self.sd[name].to(like.device, torch.float64)
        return self._dev[key]

    def lin(self, p, x):
        return F.linear(x, self.w(p + ".weight", x), self.w(p + ".bias", x))


def timestep_embedding(t, dim=256):
    """cos || sin of t * 10000^(-i / 128) (oracle.dit.timestep_embedding), in float64."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = float(t) * freqs
    return torch.cat([torch.cos(a), torch.sin(a)])[None]


def modulation(W, timestep, device="cpu"):
    """[6][C]: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp of the block at `timestep` (no micro-conditioning)."""
    e = timestep_embedding(timestep).to(device)
    emb = W.lin("adaln_single.emb.timestep_embedder.linear_2", F.silu(W.lin("adaln_single.emb.timestep_embedder.linear_1", e)))
    t6 = W.lin("adaln_single.linear", F.silu(emb))
    return W.w(P_ + "scale_shift_table", e) + t6.view(6, C)


def prompt_kv(W, y, emulate=False):
    """Raw prompts y [P][L][4096] -> the block's cross-attention K, V [P][L][C] (caption_projection: Linear -> GELU(tanh) -> Linear)."""
    r = rb if emulate else (lambda t: t)
    y = r(y.to(torch.float64))
    y1 = r(F.gelu(W.lin("caption_projection.linear_1", y), approximate="tanh"))
    y2 = r(W.lin("caption_projection.linear_2", y1))
    return r(W.lin(P_ + "attn2.to_k", y2)), r(W.lin(P_ + "attn2.to_v", y2))


def attention(q, k, v, scale, bias=None, emulate=False, chunk=1024):
    """q [B][Tq][H][D], k / v [B][Tk][H][D], bias [B][Tk] (additive, per key) -> o [B][Tq][H][D], softmax over keys, query blocks of `chunk`.
    emulate: P = exp(s - max) rounded to bf16 before PV, divided by the sum of the unrounded exponentials."""
    qh, kh, vh = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    out = torch.empty_like(qh)
    for i in range(0, qh.shape[2], chunk):
        s = (qh[:, :, i:i + chunk] @ kh.transpose(-1, -2)) * scale
        if bias is not None:
            s = s + bias[:, None, None, :]
        if emulate:
            e = torch.exp(s - s.amax(-1, keepdim=True))
            out[:, :, i:i + chunk] = (rb(e) @ vh) / e.sum(-1, keepdim=True)
        else:
            out[:, :, i:i + chunk] = torch.softmax(s, -1) @ vh
        del s
    return out.permute(0, 2, 1, 3)


def compress(W, t, n, gh, gw):
    """AttentionKVCompress.downsample_2d, 'conv' sampler (oracle.dit `compress`): depthwise 2 x 2 / stride 2 conv over the token grid, then
    LayerNorm (eps 1e-5). [n * T][C] -> [n][T / 4][C]."""
    g = t.view(n, gh, gw, C).permute(0, 3, 1, 2)
    g = F.conv2d(g, W.w(P_ + "attn1.sr.weight", t), W.w(P_ + "attn1.sr.bias", t), stride=2, groups=C)
    return F.layer_norm(g.flatten(2).transpose(1, 2), (C,), W.w(P_ + "attn1.norm.weight", t), W.w(P_ + "attn1.norm.bias", t), eps=1e-5)


def block(W, x, mod, kv, bias, n, gh, gw, emulate=False, mutation=None, chunk=1024):
    """One block on x [n * gh * gw][C] (float64): returns the new rows. mod: modulation() rows; kv: prompt_kv(); bias: [P][L] additive key bias;
    item b attends to prompt slot b % P."""
    assert mutation is None or mutation in MUTATIONS, mutation
    r = rb if emulate else (lambda t: t)
    T = gh * gw
    C = x.shape[1]          # the width of the rows given (the module's C at full width; tests/support/dit_shell_ref.py also runs toy widths)
    HEADS = C // HD
    sh1, sc1, g1, sh2, sc2, g2 = mod
    if mutation == "msa_mlp_rows_swapped":
        sh1, sc1, g1, sh2, sc2, g2 = sh2, sc2, g2, sh1, sc1, g1
    one = 0.0 if mutation == "scale_without_one" else 1.0
    scale = (1 / 8) if mutation == "softmax_scale_1_over_8" else HD ** -0.5
    # self-attention
    h = r(F.layer_norm(x, (C,), eps=1e-6) * (one + sc1) + sh1)
    q, k, v = (r(W.lin(P_ + f"attn1.to_{s}", h)) for s in "qkv")
    if W.qk_norm:
        q = r(F.layer_norm(q, (C,), W.w(P_ + "attn1.q_norm.weight", x), W.w(P_ + "attn1.q_norm.bias", x), eps=1e-5))
        k = r(F.layer_norm(k, (C,), W.w(P_ + "attn1.k_norm.weight", x), W.w(P_ + "attn1.k_norm.bias", x), eps=1e-5))
    if W.kvc:
        k, v = r(compress(W, k, n, gh, gw)), r(compress(W, v, n, gh, gw))
    q, k, v = (t.reshape(n, -1, HEADS, HD) for t in (q, k, v))
    if mutation == "v_tail_from_next_head":
        v = v.clone()
        v[:, :, 5, 64:] = v[:, :, 6, 64:]
    o = attention(q, k, v, scale, emulate=emulate, chunk=chunk)
    if mutation == "o_heads_swapped":
        o = o[:, :, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 10, 12, 13, 14, 15]]
    o = r(o.reshape(n * T, C))
    x = x + g1 * W.lin(P_ + "attn1.to_out.0", o)
    # cross-attention on the un-normalised stream
    cq = r(W.lin(P_ + "attn2.to_q", r(x))).view(n, T, HEADS, HD)
    K, V = kv
    P = K.shape[0]
    slot = [((b + 1) if mutation == "prompt_slot_shifted" else b) % P for b in range(n)]
    kb = bias.to(x.device, torch.float64)
    if mutation == "last_token_masked":
        kb = kb.clone()
        for p in range(P):
            last = int((kb[p] == kb[p].max()).nonzero().max())
            kb[p, last] = kb[p].min()
    o = attention(cq, K[slot].view(n, -1, HEADS, HD), V[slot].view(n, -1, HEADS, HD), HD ** -0.5, kb[slot], emulate, chunk)
    c = W.lin(P_ + "attn2.to_out.0", r(o.reshape(n * T, C)))
    x = x + (g1 * c if mutation == "gate_msa_on_cross" else c)
    # MLP
    h = r(F.layer_norm(x, (C,), eps=1e-6) * (one + sc2) + sh2)
    hid = r(F.gelu(W.lin(P_ + "ff.net.0.proj", h), approximate="tanh"))
    return x + g2 * W.lin(P_ + "ff.net.2", hid)


def make_prompts(P, n_tok, valid, seed, form="cli"):
    """P raw prompts [P][n_tok][4096] ~ U(-1, 1) and their additive key bias [P][n_tok]: valid[p] real tokens each. form 'cli': the 3-D mask
    the reference's CLI passes, added as is (+1 on real tokens, 0 on padding); '2d': diffusers' conversion of a 2-D mask (0 / -10000)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(P, n_tok, CAP, generator=g) * 2 - 1
    m = torch.zeros(P, n_tok)
    for p in range(P):
        m[p, :valid[p]] = 1
    return y, (m if form == "cli" else (1 - m) * -10000.0)


def make_tokens(n, T, seed):
    """Token rows [n * T][C] ~ N(0, 1) + a per-channel offset of std 0.5 (the stream is not centred): fp32 values in float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n * T, C, generator=g, dtype=torch.float64) + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()


def update_error(got_out, ref_out, x):
    """(relative L2, worst element / max |update|) of got_out - x against ref_out - x: the block's update, which the residual stream would hide."""
    gu, ru = got_out.double() - x, ref_out.double() - x
    return float((gu - ru).norm() / ru.norm()), float((gu - ru).abs().max() / ru.abs().max())
