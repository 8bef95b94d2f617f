"""float64 restatement of ONE block of the ControlLDM UNet (input_blocks.i / one layer of middle_block / output_blocks.j of UNetModel with
the options of configs/cldm.yaml), written from the operations' definitions, for the op-level tests of ir_op_unet_block
(tests/test_unet_block_ref_cpu.py, tests/test_unet_block_gpu.py):
  ResBlock._forward         GroupNorm32 (eps 1e-5) -> SiLU -> 3x3 conv, + emb_out = Linear(SiLU(time_embed(t))) per channel, GroupNorm32 -> SiLU ->
                            3x3 conv, + x (through the 1x1 skip_connection where the channel count changes)
  SpatialTransformer        GroupNorm32 (eps 1e-6), proj_in, one BasicTransformerBlock (x + attn1(norm1 x), x + attn2(norm2 x, context),
                            x + ff(norm3 x) with ff = Linear(a * gelu(g)), a | g = Linear(x)), proj_out, + the transformer's input
  Downsample / Upsample     3x3 conv, stride 2, padding 1 / nearest x2, then 3x3 conv, padding 1
  input_blocks.0            3x3 conv, padding 1
It reads nothing from the library under test; oracle/cldm.py supplies parameter names, shapes and the block layout only.

Weights: tests.golden._det.det_state_dict, one stream per block (so that a test builds only the blocks it runs), rounded to bf16 - the values
weights.pack_unet uploads - with the q and k projections of both attentions scaled by Q_GAIN so that the self-attention logits have a std of
about 3 (tests/test_unet_block_ref_cpu.py asserts that).

Rows: [n * h * w][C] float64, item-major, pixel-major within an item (NHWC). Every function runs on the device of its inputs; the attention is
chunked by query blocks so that 4096 tokens fit.

`emulate=True` rounds to bf16 where the HIP path (ures / uxf / ublock in csrc/api.cpp) stores bf16: every activation between kernels, the
normalised rows, q | k | v and the cached context K / V, P before PV, the attention outputs, the GEGLU inputs and product and the bf16 copy of
the stream proj_out reads; the token stream inside the transformer and the time embedding are rounded to fp32. `mutation` plants one bug
(MUTATIONS), to show that the gates see it.

GATES: per block kind (rel-L2 of the output, worst element / max |ref| of the output, and the same two of the update where the block has an
identity residual: out - x for a ResBlock with cin == cout, out - (the transformer's input) for a block with a transformer and no resample)
= 2 x EMULATION, the largest bf16-emulation error of that kind over the cases of tests/test_unet_block_gpu.py, measured in float64 on the
CPU by tests/test_unet_block_ref_cpu.py and rounded up to two digits. No figure comes from the HIP output."""
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import cldm as ocldm
from tests.golden._det import det_state_dict
from tests.support.vae_segment_ref import conv2d

CFG = dict(ocldm.DEFAULT_CFG)   # configs/cldm.yaml: 320 x (1, 2, 4, 4), 2 res blocks, heads of 64, context 1024
N_TOK = 77
TIMESTEP = 400.0
Q_GAIN = 3.0 ** 0.5
MUTATIONS = ("emb_out_dropped", "emb_out_other_timestep", "shortcut_dropped", "softmax_scale_missing", "cross_attends_tokens", "geglu_halves_swapped",
             "norm2_norm3_swapped", "proj_out_residual_after_norm", "down_pad_0101", "up_shifted", "decoder_slices_swapped")
OTHER_TIMESTEP = 999.0

# kind: (rel-L2 out, worst out, rel-L2 update, worst update) of the bf16 emulation (None: the kind has no identity residual); see the docstring
EMULATION = {
    "conv0": (1.7e-3, 2.0e-3, None, None),        # measured 1.66e-3, 1.99e-3
    "down": (1.7e-3, 2.9e-3, None, None),         # 1.67e-3, 2.83e-3 (the 1280-wide one)
    "res": (2.2e-3, 3.5e-3, 4.8e-3, 6.4e-3),      # 2.16e-3, 3.41e-3, 4.74e-3, 6.32e-3
    "res_sc": (2.7e-3, 4.4e-3, None, None),       # 2.64e-3, 4.39e-3
    "res_up": (3.2e-3, 3.9e-3, None, None),       # 3.10e-3, 3.82e-3
    "xf": (4.1e-3, 4.1e-3, 5.2e-3, 4.7e-3),       # 4.02e-3, 4.09e-3, 5.14e-3, 4.65e-3
    "res_xf": (5.2e-3, 6.2e-3, 7.2e-3, 8.6e-3),   # 5.18e-3, 6.11e-3 (ragged_1280), 7.10e-3, 8.57e-3 (out6)
    "res_xf_up": (5.5e-3, 5.9e-3, None, None),    # 5.42e-3, 5.81e-3
}
MARGIN = 2.0
GATES = {k: tuple(None if e is None else MARGIN * e for e in v) for k, v in EMULATION.items()}


# The cases of tests/test_unet_block_gpu.py: id -> (set, index, n, h, w), h x w the resolution entering the block. Every distinct block shape
# once on 8 x 8, the token counts of a 512-px image, a ragged grid (240 tokens, no multiple of 64) and two batches.
CASES = {
    "in0_conv": (0, 0, 1, 8, 8), "in1_xf320": (0, 1, 1, 8, 8), "in4_320to640_xf": (0, 4, 1, 8, 8), "in5_xf640": (0, 5, 1, 8, 8),
    "in7_640to1280_xf": (0, 7, 1, 8, 8), "in8_xf1280": (0, 8, 1, 8, 8), "in10_res1280": (0, 10, 1, 8, 8),
    "in3_down320": (0, 3, 1, 8, 8), "in6_down640": (0, 6, 1, 8, 8), "in9_down1280": (0, 9, 1, 8, 8),
    "mid0_res": (1, 0, 1, 8, 8), "mid1_xf": (1, 1, 1, 8, 8), "mid2_res": (1, 2, 1, 8, 8),
    "out0_2560to1280": (2, 0, 1, 8, 8), "out2_2560to1280_up": (2, 2, 1, 8, 8), "out3_2560to1280_xf": (2, 3, 1, 8, 8),
    "out5_1920to1280_xf_up": (2, 5, 1, 8, 8), "out6_1920to640_xf": (2, 6, 1, 8, 8), "out7_1280to640_xf": (2, 7, 1, 8, 8),
    "out8_960to640_xf_up": (2, 8, 1, 8, 8), "out9_960to320_xf": (2, 9, 1, 8, 8), "out10_640to320_xf": (2, 10, 1, 8, 8),
    "product_320_64x64": (0, 1, 1, 64, 64), "product_640_32x32": (0, 5, 1, 32, 32), "product_1280_16x16": (0, 8, 1, 16, 16),
    "ragged_320": (0, 2, 1, 12, 20), "ragged_640": (2, 7, 1, 12, 20), "ragged_1280": (2, 4, 1, 12, 20),
    "ragged_up": (2, 8, 1, 12, 20), "ragged_down": (0, 3, 1, 12, 20),
    "batch_xf": (0, 5, 2, 8, 8), "batch_up": (2, 5, 2, 8, 8),
}


def case_inputs(W, case):
    """(x rows [n * h * w][cin] float64 of bf16 values, cin, cout, kind, scale) of a case."""
    set_, index, n, h, w = CASES[case]
    cin, cout, kind, scale = block_io(W.cfg, set_, index)
    return make_rows(n, h * w, cin, seed=zlib.crc32(case.encode()) % 100000), cin, cout, kind, scale


def rb(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def r32(t):
    return t.to(torch.float32).to(t.dtype)


def _layout(cfg):
    return ocldm.layout(cfg, bool(cfg.get("control")))


def block_layers(cfg, set_, index):
    """[(parameter prefix, layer tuple of oracle.cldm.layout)] of block `index` of set 0 (input_blocks), 1 (middle_block: one layer each) or 2."""
    inb, mid_ch, outb, _ = _layout(cfg)
    if set_ == 0:
        return [(f"input_blocks.{index}.{k}", L) for k, L in enumerate(inb[index])]
    if set_ == 1:
        return [(f"middle_block.{index}", (("res", mid_ch, mid_ch), ("xf", mid_ch), ("res", mid_ch, mid_ch))[index])]
    return [(f"output_blocks.{index}.{k}", L) for k, L in enumerate(outb[index])]


def block_counts(cfg):
    inb, _, outb, _ = _layout(cfg)
    return len(inb), 3, len(outb)


def block_io(cfg, set_, index):
    """(cin, cout, kind, scale) of a block: scale 2 / -2: the grid doubles / halves."""
    layers = [L for _, L in block_layers(cfg, set_, index)]
    names = [L[0] for L in layers]
    first, last = layers[0], layers[-1]
    cin = first[1]
    cout = first[2] if first[0] in ("conv", "res") else first[1]
    if names == ["conv"]:
        return cin, cout, "conv0", 1
    if names == ["down"]:
        return cin, cout, "down", -2
    if names == ["xf"]:
        return cin, cout, "xf", 1
    kind = "res" + ("_xf" if "xf" in names else "") + ("_up" if "up" in names else "")
    if kind == "res" and cin != cout:
        kind = "res_sc"
    return cin, cout, kind, 2 if last[0] == "up" else 1


class UNetWeights:
    """The UNet (cfg['control']: the ControlNet) of `cfg` with deterministic bf16-rounded weights under the reference's parameter names,
    generated block by block - or, with `sd`, a given state dict as it is."""

    def __init__(self, cfg=None, seed=727, q_gain=Q_GAIN, sd=None):
        self.cfg = dict(CFG, **(cfg or {}))
        self.hd = self.cfg["num_head_channels"]
        self.seed, self.q_gain = seed, q_gain
        self.shapes = ocldm.state_dict_shapes(self.cfg, bool(self.cfg.get("control")))
        self.sd, self._dev = dict(sd or {}), {}

    @staticmethod
    def group(name):
        p = name.split(".")
        return ".".join(p[:2]) if p[0] in ("input_blocks", "middle_block", "output_blocks") else p[0]

    def need(self, group):
        if any(self.group(k) == group for k in self.sd):
            return
        sd = det_state_dict({k: s for k, s in self.shapes.items() if self.group(k) == group}, seed=self.seed + zlib.crc32(group.encode()) % 100000)
        for k, v in sd.items():
            if any(t in k for t in ("attn1.to_q.", "attn1.to_k.", "attn2.to_q.", "attn2.to_k.")):
                v = v * self.q_gain
            self.sd[k] = rb(v)

    def full_sd(self):
        for g in sorted({self.group(k) for k in self.shapes}):
            self.need(g)
        return self.sd

    def w(self, name, like):
        """Tensor `name` in float64 on the device of `like` (cached per device)."""
        key = (name, like.device)
        if key not in self._dev:
            self.need(self.group(name))
            self._dev[key] = self.sd[name].to(like.device, torch.float64)
        return self._dev[key]

    def drop_device_copies(self):
        self._dev.clear()

    def lin(self, p, x, bias=True):
        return F.linear(x, self.w(p + ".weight", x), self.w(p + ".bias", x) if bias else None)


def time_emb(W, t, device="cpu", emulate=False):
    """emb [temb] = time_embed(timestep_embedding(t)): cos || sin of t * 10000^(-i / half), Linear, SiLU, Linear."""
    mc = W.cfg["model_channels"]
    half = mc // 2
    a = float(t) * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    e = torch.cat([torch.cos(a), torch.sin(a)]).to(device)
    f = r32 if emulate else (lambda v: v)
    return f(W.lin("time_embed.2", f(F.silu(W.lin("time_embed.0", f(e))))))


def rows_to_nchw(x, n, h, w):
    return x.view(n, h, w, -1).permute(0, 3, 1, 2)


def nchw_to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _conv3(W, p, x, stride=1, padding=1):
    return conv2d(x, W.w(p + ".weight", x), W.w(p + ".bias", x), stride=stride, padding=padding)


def _gn(W, p, x, eps):
    return F.group_norm(x, 32, W.w(p + ".weight", x), W.w(p + ".bias", x), eps=eps)


def res_block(W, p, x, emb, emulate=False, mutation=None, emb_other=None):
    """ResBlock._forward on x NCHW; emb: time_emb()."""
    r = rb if emulate else (lambda t: t)
    e = emb_other if mutation == "emb_out_other_timestep" else emb
    emb_out = W.lin(p + ".emb_layers.1", F.silu(e))
    if emulate:
        emb_out = r32(emb_out)
    if mutation == "emb_out_dropped":
        emb_out = torch.zeros_like(emb_out)
    h = r(F.silu(_gn(W, p + ".in_layers.0", x, 1e-5)))
    h = r(_conv3(W, p + ".in_layers.2", h) + emb_out[None, :, None, None])
    h = r(F.silu(_gn(W, p + ".out_layers.0", h, 1e-5)))
    if p + ".skip_connection.weight" in W.shapes:
        skip = r(conv2d(x, W.w(p + ".skip_connection.weight", x), W.w(p + ".skip_connection.bias", x)))
        if mutation == "shortcut_dropped":
            skip = torch.zeros_like(skip)
    else:
        skip = x
    return r(_conv3(W, p + ".out_layers.3", h) + skip)


def attention(q, k, v, heads, scale, emulate=False, chunk=1024):
    """q [B][Tq][C], k / v [B][Tk][C] -> [B][Tq][C]: softmax(q k^T * scale) v per head, query blocks of `chunk`.
    emulate: P = exp(s - max) rounded to bf16 before PV, divided by the sum of the unrounded exponentials."""
    B, Tq, C = q.shape
    d = C // heads
    qh, kh, vh = (t.reshape(B, -1, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
    out = torch.empty_like(qh)
    for i in range(0, Tq, chunk):
        s = (qh[:, :, i:i + chunk] @ kh.transpose(-1, -2)) * scale
        if emulate:
            e = torch.exp(s - s.amax(-1, keepdim=True))
            out[:, :, i:i + chunk] = (rb(e) @ vh) / e.sum(-1, keepdim=True)
        else:
            out[:, :, i:i + chunk] = torch.softmax(s, -1) @ vh
        del s
    return out.permute(0, 2, 1, 3).reshape(B, Tq, C)


def _ln(W, p, x):
    return F.layer_norm(x, (x.shape[-1],), W.w(p + ".weight", x), W.w(p + ".bias", x), eps=1e-5)


def spatial_transformer(W, p, x, context, emulate=False, mutation=None, chunk=1024, probe=None):
    """SpatialTransformer.forward on x NCHW with context [n_tok][ctx_dim] (one prompt for the batch)."""
    r = rb if emulate else (lambda t: t)
    f = r32 if emulate else (lambda t: t)
    n, C, H, Wd = x.shape
    heads = C // W.hd
    t = p + ".transformer_blocks.0"
    scale = 1.0 if mutation == "softmax_scale_missing" else W.hd ** -0.5
    n1, n2, n3 = (t + ".norm1", t + ".norm3", t + ".norm2") if mutation == "norm2_norm3_swapped" else (t + ".norm1", t + ".norm2", t + ".norm3")
    g = r(_gn(W, p + ".norm", x, 1e-6))
    h = f(W.lin(p + ".proj_in", nchw_to_rows(g).view(n, H * Wd, C)))
    # attn1
    xn = r(_ln(W, n1, h))
    q, k, v = (r(W.lin(f"{t}.attn1.to_{s}", xn, bias=False)) for s in "qkv")
    if probe is not None:
        probe["self_logit_std"] = float(((q.view(n, -1, heads, W.hd)[0, :64].permute(1, 0, 2) @ k.view(n, -1, heads, W.hd)[0].permute(1, 2, 0)) * scale).std())
    h = f(h + W.lin(t + ".attn1.to_out.0", r(attention(q, k, v, heads, scale, emulate, chunk))))
    # attn2
    xn = r(_ln(W, n2, h))
    q = r(W.lin(t + ".attn2.to_q", xn, bias=False))
    if mutation == "cross_attends_tokens":   # the normalised tokens in the context's place (cut or zero-padded to its width)
        cd = W.cfg["context_dim"]
        src = xn[..., :cd] if C >= cd else F.pad(xn, (0, cd - C))
    else:
        src = r(context.to(x.dtype))[None].expand(n, -1, -1)
    k, v = r(W.lin(t + ".attn2.to_k", src, bias=False)), r(W.lin(t + ".attn2.to_v", src, bias=False))
    h = f(h + W.lin(t + ".attn2.to_out.0", r(attention(q, k, v, heads, scale, emulate, chunk))))
    # GEGLU feed-forward
    xn = r(_ln(W, n3, h))
    a, gte = r(W.lin(t + ".ff.net.0.proj", xn)).chunk(2, dim=-1)
    if mutation == "geglu_halves_swapped":
        a, gte = gte, a
    h = f(h + W.lin(t + ".ff.net.2", r(a * F.gelu(gte))))
    y = W.lin(p + ".proj_out", r(h)).view(n, H, Wd, C).permute(0, 3, 1, 2)
    return r(y + (g if mutation == "proj_out_residual_after_norm" else x))


def block(W, set_, index, x, n, h, w, emb, context, emulate=False, mutation=None, chunk=1024, emb_other=None, probe=None):
    """One block on rows x [n * h * w][cin] (float64, bf16 values): returns (rows of the output, rows of the transformer's input or None)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    r = rb if emulate else (lambda t: t)
    if mutation == "decoder_slices_swapped":   # [h | skip] read as [skip | h]
        assert set_ == 2
        skips = _layout(W.cfg)[3]
        hch = x.shape[1] - skips[len(skips) - 1 - index]
        x = torch.cat([x[:, hch:], x[:, :hch]], dim=1)
    cur, base = rows_to_nchw(x, n, h, w), None
    for p, L in block_layers(W.cfg, set_, index):
        if L[0] == "conv":
            cur = r(_conv3(W, p, cur))
        elif L[0] == "res":
            cur = res_block(W, p, cur, emb, emulate, mutation, emb_other)
        elif L[0] == "xf":
            base = nchw_to_rows(cur)
            cur = spatial_transformer(W, p, cur, context, emulate, mutation, chunk, probe)
        elif L[0] == "down":
            if mutation == "down_pad_0101":
                cur = r(_conv3(W, p + ".op", F.pad(cur, (0, 1, 0, 1)), stride=2, padding=0))
            else:
                cur = r(_conv3(W, p + ".op", cur, stride=2))
        elif L[0] == "up":
            up = cur.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
            if mutation == "up_shifted":
                up = torch.cat([up[:, :, :, :1], up[:, :, :, :-1]], dim=3)
            cur = r(_conv3(W, p + ".conv", up))
            base = None
    return nchw_to_rows(cur), base


def update_base(W, set_, index, x, base):
    """What the update of a block is measured against: the transformer's input, x of a ResBlock that keeps its channel count, or None."""
    cin, cout, kind, _ = block_io(W.cfg, set_, index)
    if kind in ("xf", "res_xf"):
        return base
    return x if kind == "res" else None


def make_rows(n, hw, c, seed):
    """Rows [n * hw][c] ~ N(0, 1) + a per-channel offset of std 0.5, bf16 values in float64."""
    g = torch.Generator().manual_seed(seed)
    return rb(torch.randn(n * hw, c, generator=g, dtype=torch.float64) + 0.5 * torch.randn(c, generator=g, dtype=torch.float64))


def make_context(W, seed=93):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N_TOK, W.cfg["context_dim"], generator=g) * 2 - 1).double()


def errors(got, ref, base=None):
    """(rel-L2, worst / max |ref|) of the output, then the same of the update against `base` (None, None without one)."""
    got, ref = got.double(), ref.double()
    d = got - ref
    out = [float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())]
    if base is None:
        return tuple(out) + (None, None)
    ru = ref - base.double()
    return tuple(out) + (float(d.norm() / ru.norm()), float(d.abs().max() / ru.abs().max()))


def inside(err, gate):
    return all(g is None or e <= g for e, g in zip(err, gate))


def outside_by(err, gate):
    """The largest error / gate ratio over the measures."""
    return max(e / g for e, g in zip(err, gate) if g is not None)


def device_weights(sd):
    """A state dict with the tensors the device keeps in bf16 (every matrix but the time-embedding ones) rounded to bf16."""
    return {k: (rb(v) if v.dim() >= 2 and "emb_layers" not in k and "time_embed" not in k else v) for k, v in sd.items()}


def network(Wu, Wc, zT, c_latent, context, t, emulate=False):
    """Reflow_ControlLDM.sample_log chained from block(): zT + UNet(zT, t, context, control = ControlNet(cat(zT, c_latent))) on NCHW float64
    latents (Wc / c_latent None: the UNet alone). emulate: the rounding points of cldm_run() on top of the blocks' (the bf16 input rows,
    zero_conv_i(g_i) + hs_i and the h of the first decoder block as bf16, the last GroupNorm + SiLU as bf16, the last conv in fp32)."""
    r = rb if emulate else (lambda v: v)
    n, _, h, w = zT.shape
    nin, nmid, nout = block_counts(Wu.cfg)

    def encoder(W, x):
        emb = time_emb(W, t, emulate=emulate)
        hs, H, Wd, cur = [], h, w, r(nchw_to_rows(x))
        for i in range(nin):
            cur, _ = block(W, 0, i, cur, n, H, Wd, emb, context, emulate)
            if block_io(W.cfg, 0, i)[3] == -2:
                H, Wd = H // 2, Wd // 2
            hs.append((cur, H, Wd))
        mid = cur
        for k in range(nmid):
            mid, _ = block(W, 1, k, mid, n, H, Wd, emb, context, emulate)
        return hs, mid, emb

    hs, mid, emb = encoder(Wu, zT)
    if Wc is not None:
        gs, gmid, _ = encoder(Wc, torch.cat([zT, c_latent], dim=1))
        def zero(p, g):   # a 1x1 conv over rows
            return F.linear(g, Wc.w(p + ".weight", g).flatten(1), Wc.w(p + ".bias", g))

        hs = [(r(hc + zero(f"zero_convs.{i}.0", g)), H, Wd) for i, ((hc, H, Wd), (g, _, _)) in enumerate(zip(hs, gs))]
        mid = r(mid + zero("middle_block_out.0", gmid))
    cur, (_, H, Wd) = mid, hs[-1]
    for j in range(nout):
        skip, _, _ = hs.pop()
        cur, _ = block(Wu, 2, j, torch.cat([cur, skip], dim=1), n, H, Wd, emb, context, emulate)
        if block_io(Wu.cfg, 2, j)[3] == 2:
            H, Wd = 2 * H, 2 * Wd
    y = r(F.silu(_gn(Wu, "out.0", rows_to_nchw(cur, n, H, Wd), 1e-5)))
    v = _conv3(Wu, "out.2", y)
    return zT + (r32(v) if emulate else v)


# ---- each control residual alone (tests/test_cldm_gpu.py::test_each_control_residual_alone): CLDM_SMALL, a ControlNet whose zero-convs are
# all zero except number i, sample_log with control minus sample_log without, against the same difference of oracle/cldm.py.
CLDM_SMALL = dict(model_channels=64, channel_mult=(1, 2, 4, 4), num_res_blocks=2, attention_resolutions=(4, 2, 1), num_head_channels=32,
                  context_dim=64, in_channels=4, hint_channels=4, out_channels=4)
N_RESIDUALS = 13
RESIDUAL_SEEDS = dict(unet=707, cnet=708, zT=61, c_latent=62, context=63)   # the weights of test_cldm_gpu.make_cldm, a 16 x 16 latent
# rel-L2 of (emulated difference - oracle difference) / oracle difference per residual, measured by tests/test_unet_block_ref_cpu.py on
# the CPU (rounded up to two digits); the gate is MARGIN times it. The rounding noise of the two runs is about the same for every i, so the
# figure grows as the residual's own effect shrinks (17 % of the output for residual 0, 3.5 % for number 12); no residual needed its zero-conv
# scaled: the widest gate is 0.32, and a residual that is lost or lands in another slice gives 1.0 or more.
RESIDUAL_EMULATION = (1.9e-2, 2.2e-2, 2.8e-2, 3.3e-2, 2.9e-2, 4.1e-2, 5.4e-2, 4.5e-2, 5.6e-2, 8.9e-2, 1.4e-1, 1.5e-1, 1.6e-1)
#            measured  1.88e-2 2.11e-2 2.77e-2 3.25e-2 2.86e-2 4.06e-2 5.32e-2 4.46e-2 5.54e-2 8.87e-2 1.33e-1 1.48e-1 1.51e-1
RESIDUAL_GATES = tuple(MARGIN * e for e in RESIDUAL_EMULATION)


def only_residual(sd_c, i):
    """The ControlNet state dict sd_c with every zero-conv (zero_convs.0 .. 11, middle_block_out = number 12) zeroed except number i."""
    keep = f"zero_convs.{i}.0." if i < N_RESIDUALS - 1 else "middle_block_out.0."
    return {k: (torch.zeros_like(v) if k.startswith(("zero_convs.", "middle_block_out.")) and not k.startswith(keep) else v) for k, v in sd_c.items()}


def residual_inputs():
    from tests.golden._det import det_input
    s = RESIDUAL_SEEDS
    return (det_input(s["zT"], (1, 4, 16, 16), -2.0, 2.0), det_input(s["c_latent"], (1, 4, 16, 16), -2.0, 2.0),
            det_input(s["context"], (1, N_TOK, CLDM_SMALL["context_dim"]), -1.0, 1.0))
