"""fp32 restatement of ONE SwinTransformerBlock behind its qkv projection (oracle/swinir.py _block from the qkv tensor on), on the device
layouts of the fused kernels in csrc/swin_fused.hip (swin_block_kernel, swin_attn_proj_kernel, swin_mlp_kernel).

Weights: tests.golden._det.det_state_dict, rounded to bf16, packed by the production weights.pack_swinir - so proj_t, biasT / biasM, mlp_t,
mlp_v and qkv_t are exactly what the model uploads, and the reference reads the same (bf16-exact) values. Token rows: [T][192] fp32, channels
C..191 zero; qkv rows: [T][576] bf16 values in the device layout (q | k | v x 6 heads x 32, head columns hd..31 zero). T = B * H * W, image-major.

`emulate=True` rounds to bf16 where the kernels do (LN outputs, the unnormalised P, O after 1 / sum, the GELU hidden units, the next block's
LN1 and qkv rows): the CPU test uses it to show that the GPU gates sit well above bf16 noise. `mutation` plants one layout bug, to show that
the gates see it (tests/test_swin_block_ref_cpu.py)."""
from fractions import Fraction

import torch
import torch.nn.functional as F

from instarevive_amd import weights as Wt
from oracle import swinir as oswin
from tests.golden._det import det_state_dict

CP, LDQ, HEADS, WS = 192, 576, 6, 8
MUTATIONS = ("bias_transposed", "ln_over_192", "v_heads_swapped", "class3_unmasked", "roll_reversed", "fc2_bias_dropped")


def rb(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bits_to_f32(bits):
    return bits.contiguous().view(torch.bfloat16).to(torch.float32)


class BlockWeights:
    """An RSTB of three blocks (block 0 unshifted, block 1 shifted, each with a next block that has qkv_t) of embed_dim C and `hid` hidden
    units: `sd` holds the bf16-rounded reference tensors, `packed` the production device tensors."""

    def __init__(self, C=180, hid=360, seed=7, bias_gain=1.0):
        assert C % HEADS == 0 and C // HEADS <= 32
        self.C, self.hid, self.hid_p, self.hd = C, hid, Wt.pad_to(hid, 32), C // HEADS
        self.cfg = dict(oswin.DEFAULT_CFG, embed_dim=C, depths=[3], num_heads=[HEADS], mlp_ratio=Fraction(hid, C))
        sd = det_state_dict(oswin.state_dict_shapes(self.cfg), seed=seed)
        for k in sd:
            if k.endswith("relative_position_bias_table"):
                sd[k] = sd[k] * bias_gain
        self.sd = {k: rb(v) for k, v in sd.items()}
        self.packed = Wt.pack_swinir(self.sd, self.cfg)
        self.rpi = oswin._relative_position_index(WS)

    def p(self, j):
        return f"layers.0.residual_group.blocks.{j}."

    def d(self, j):
        return f"swin.l0.b{j}."

    def qkv_dev(self, j):
        """Block j's qkv weight [576][192] and bias [576] in the device layout (fp32 values of the packed bf16)."""
        return bits_to_f32(self.packed[self.d(j) + "qkv.w"]), self.packed[self.d(j) + "qkv.b"]


def layer_norm_rows(x, g, b, C, n=None):
    """LayerNorm over the first C (or, as a planted bug, n) channels of [T][192] rows; the result is zero beyond C, as the kernels write it."""
    n = C if n is None else n
    gp, bp = torch.zeros(CP), torch.zeros(CP)
    gp[:C], bp[:C] = g, b
    return F.pad(F.layer_norm(x[:, :n], (n,), None, None, 1e-5) * gp[:n] + bp[:n], (0, CP - n))


def qkv_rows(ln, w, b):
    """[T][192] normalised rows (bf16 values) times the device-layout qkv weight: [T][576]."""
    return ln @ w.t() + b


def attention_half(W, j, qkv, x, B, H, Wd, shift, emulate=False, mutation=None):
    """x + proj(W-MSA(q, k, v)) + proj bias: the row after the first residual (swinir.py:258-283), [T][192]."""
    C, hd, sd, p = W.C, W.hd, W.sd, W.p(j)
    q, k, v = (qkv[:, i * CP:(i + 1) * CP].reshape(B, H, Wd, HEADS, 32)[..., :hd] for i in range(3))
    if mutation == "v_heads_swapped":
        v = v[..., [0, 2, 1, 3, 4, 5], :]
    s = -shift if mutation != "roll_reversed" else shift
    if shift:
        q, k, v = (torch.roll(t, (s, s), (1, 2)) for t in (q, k, v))
    q, k, v = (oswin._partition(t.reshape(B, H, Wd, HEADS * hd), WS).reshape(-1, 64, HEADS, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)                                     # [win][head][query][key]
    bias = sd[p + "attn.relative_position_bias_table"][W.rpi.view(-1)].view(64, 64, -1).permute(2, 0, 1)
    if mutation == "bias_transposed":
        bias = bias.transpose(-2, -1)
    attn = attn + bias[None]
    if shift:
        mask = oswin.shift_mask(H, Wd, WS, shift)                                     # [window][query][key]
        if mutation == "class3_unmasked":
            mask = mask.clone()
            mask[-1] = 0.0                                                             # the bottom-right window: last row and last column
        nW = mask.shape[0]
        attn = (attn.view(B, nW, HEADS, 64, 64) + mask[None, :, None]).view(-1, HEADS, 64, 64)
    if emulate:   # the kernel: P = exp(s - max) in bf16, O = bf16((P V) / sum of the unrounded exponentials)
        e = torch.exp(attn - attn.amax(-1, keepdim=True))
        o = rb((rb(e) @ v) / e.sum(-1, keepdim=True))
    else:
        o = attn.softmax(-1) @ v
    o = o.transpose(1, 2).reshape(-1, 64, C)
    o = F.linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
    h = oswin._reverse(o, WS, H, Wd)
    if shift:
        h = torch.roll(h, (-s, -s), (1, 2))
    return x + F.pad(h.reshape(-1, C), (0, CP - C))


def mlp_half(W, j, x, emulate=False, mutation=None):
    """x + fc2(GELU(fc1(LN2(x)))) (swinir.py:289), [T][192]."""
    C, sd, p = W.C, W.sd, W.p(j)
    n = CP if mutation == "ln_over_192" else None
    m = layer_norm_rows(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"], C, n)[:, :C]
    if emulate:
        m = rb(m)
    hid = F.gelu(F.linear(m, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
    if emulate:
        hid = rb(hid)
    b2 = sd[p + "mlp.fc2.bias"]
    if mutation == "fc2_bias_dropped":
        b2 = b2.clone()
        b2[int(b2.abs().argmax())] = 0.0
    return x + F.pad(F.linear(hid, sd[p + "mlp.fc2.weight"], b2), (0, CP - C))


def next_rows(W, j, x, emulate=False, mutation=None):
    """The next block's norm1 rows [T][192] and qkv rows [T][576] from the new residual rows x."""
    C, sd, p = W.C, W.sd, W.p(j + 1)
    n = CP if mutation == "ln_over_192" else None
    ln = layer_norm_rows(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"], C, n)
    if emulate:
        ln = rb(ln)
    qkv = qkv_rows(ln, *W.qkv_dev(j + 1))
    return ln, (rb(qkv) if emulate else qkv)


def block(W, j, qkv, x, B, H, Wd, shift, emulate=False, mutation=None):
    """Block j (shift 0 or 4) from its qkv rows and input rows: dict(attn=post-attention rows, out=block output, ln1 / qkv=the next block's)."""
    a = attention_half(W, j, qkv, x, B, H, Wd, shift, emulate, mutation)
    out = mlp_half(W, j, a, emulate, mutation)
    ln1, nq = next_rows(W, j, out, emulate, mutation)
    return dict(attn=a, out=out, ln1=ln1, qkv=nq)


def make_inputs(W, j, B, H, Wd, seed, q_gain=1.0):
    """Residual rows x ~ N(0, 1) (zero beyond C) and block j's qkv rows from them - norm1 + qkv projection, as the model makes them - rounded to
    bf16; q_gain scales the q columns (peaky scores)."""
    g = torch.Generator().manual_seed(seed)
    T = B * H * Wd
    x = torch.zeros(T, CP)
    x[:, :W.C] = torch.randn(T, W.C, generator=g)
    p = W.p(j)
    ln = rb(layer_norm_rows(x, W.sd[p + "norm1.weight"], W.sd[p + "norm1.bias"], W.C))
    qkv = qkv_rows(ln, *W.qkv_dev(j))
    qkv[:, :CP] *= q_gain
    return x, rb(qkv)


def update_error(got_out, ref_out, x):
    """(relative L2, worst element / max |update|) of got_out - x against ref_out - x: the block's update, which the residual stream would hide."""
    gu, ru = got_out - x, ref_out - x
    return float((gu - ru).norm() / ru.norm()), float((gu - ru).abs().max() / ru.abs().max())
