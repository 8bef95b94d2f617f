"""float64 restatement of a SEGMENT of the VAE chain (oracle/vae.py's _resnet, _attn and the Downsample / Upsample lines of vae_encode_mean /
vae_decode), for the op-level tests of ir_op_vae_segment (tests/test_vae_segment_ref_cpu.py, tests/test_vae_segment_gpu.py).

Steps of a half, in production order (`steps(half)`; the library's ir_op_vae_segment_info reports the same names):
    decoder (half 1)  mid.res0, mid.attn, mid.res1, up3.res0, up3.res1, up3.res2, up3.us, up2.res0, ... , up0.res2
    encoder (half 0)  down0.res0, down0.res1, down0.ds, ... , down3.res1, mid.res0, mid.attn, mid.res1

Weights (`weights(kind)`): tests.golden._det.det_state_dict of the full-width model (ch 128, ch_mult (1, 2, 4, 4), 2 / 3 blocks per level), with
gains so that a block is not trivially flat - RES_GAIN * RES_GROWTH ** i on the conv2 of the i-th ResnetBlock of a half (the stream grows along
the chain; the branch h keeps an rms between 0.5x and 2x that of the skip path), QK_GAIN on the attention's to_q / to_k (logit std about 3: softmax is not uniform) and V_GAIN on its to_out - and then rounded to
bf16, the values the production path uploads. kind "peaky": logits scaled PEAKY_GAIN further (std about 18); with make_input(spike=True) the
last 32 keys then score +- 100 and more. The bf16 d = 512 kernel follows any such jump by moving its softmax reference in place (its overflow
flag cannot be raised by scores), but the fp8 d = 512 kernel gives such queries up and raises its flag: that is the GPU test's way into
attnblock()'s fallback chain. tests/test_vae_segment_ref_cpu.py asserts the rms ratios and the logit spread.

`segment(sd, half, first, count, x)`: x [N][C][H][W] (NCHW, any float dtype: the arithmetic runs in x's dtype on x's device, GroupNorm statistics
and the attention core always in float64).
  emulate=True rounds to bf16 wherever the HIP path stores bf16: every conv / linear output after bias and residual, the GroupNorm (+ SiLU) output
    - as a stored tensor and when it is made inside the NORM conv alike -, q / k / v / o, P; statistics come from the stored conv output.
  fp8=True (with emulate) restates the fp8 branch of resblock(): both GroupNorm + SiLU outputs as e4m3(x * 16), both 3x3 convs on e4m3 weights
    quantised per output channel (weights.pack_conv3x3_fp8), exact accumulation.
  mutation=<name> plants one bug (MUTATIONS).
  tape=Tape(): the first call records every GroupNorm's statistics and the attention's k / v; a later call with the same tape on a ROW BAND of x
    replays them, so that a band can be evaluated in float64 with the statistics of the full-size pass (the GPU test's certification).
  Returns (out, skip): skip = the skip path of the LAST step when that is a ResnetBlock or the AttnBlock (x, or conv_shortcut(x)), else None.

GATES, per segment kind: (rel-L2, worst / range) of the whole output, of its border frame (outermost pixel ring) and - for a segment ending in a
block - of the last block's update (out - skip, skip from the reference). Derived in tests/test_vae_segment_ref_cpu.py: bf16 (or fp8) emulation
against float64 on 16 x 24 (512-channel segments) or 32 x 48 maps, times 2, rounded up to one digit. Measured emulation values:
    kind            whole             border            update
    dec_l0          5.9e-3  3.5e-3    5.5e-3  1.9e-3    8.8e-3  1.0e-2
    dec_l1          4.9e-3  2.8e-3    4.6e-3  1.7e-3    7.0e-3  7.6e-3
    dec_l32         7.2e-3  4.7e-3    6.6e-3  1.6e-3    1.1e-2  1.4e-2
    dec_mid         6.6e-3  4.4e-3    5.8e-3  2.5e-3    1.1e-2  1.5e-2
    enc_l01         5.8e-3  3.3e-3    5.6e-3  2.2e-3    8.6e-3  8.2e-3
    enc_l23mid      5.9e-3  3.7e-3    5.6e-3  2.7e-3    5.4e-2  5.2e-2   (the encoder's attention update is 0.14 of its input: a small denominator)
    dec_mid_peaky   1.5e-2  3.0e-2    1.3e-2  2.6e-2    7.8e-2  3.5e-1   (spiked keys: logits of +- 100 and more magnify the bf16 rounding of q and k)
    dec_l0_fp8      7.0e-2  4.1e-2    6.4e-2  2.0e-2    1.0e-1  1.2e-1
    dec_l32_fp8     9.0e-2  5.0e-2    8.0e-2  1.8e-2    1.4e-1  1.4e-1
    enc_l01_fp8     7.0e-2  4.1e-2    6.6e-2  2.9e-2    1.0e-1  1.0e-1
Checked at the GPU cases' sizes: the same emulation (float64, or against the certified fp32 pass above 600 x 600) on the MI355X for every case
of tests/test_vae_segment_gpu.py, because `worst` metrics are maxima and grow with the map. Largest emulation figure per kind over its cases:
    dec_l0          5.6e-3  3.4e-3    5.2e-3  1.7e-3    8.7e-3  1.0e-2
    dec_l1          4.7e-3  3.05e-3   4.4e-3  1.6e-3    6.9e-3  8.6e-3      worst above the CPU's 2.8e-3 -> gate 7e-3 instead of 6e-3
    dec_l32         7.2e-3  4.5e-3    6.7e-3  1.94e-3   1.1e-2  1.2e-2
    dec_mid         5.5e-3  4.5e-3    4.8e-3  2.6e-3    8.9e-3  1.6e-2
    enc_l01         5.5e-3  3.2e-3    5.3e-3  2.1e-3    8.4e-3  9.76e-3
    enc_l23mid      5.6e-3  3.7e-3    5.2e-3  2.4e-3    6.8e-2  6.0e-2
    dec_mid_peaky   3.5e-2  1.9e-1    5.3e-2  1.9e-1    3.1e-1  3.5e+0     at 64 x 64 -> the gates in force
    dec_l0_fp8      6.6e-2  3.7e-2    5.9e-2  1.7e-2    1.0e-1  1.1e-1
    dec_l32_fp8     8.4e-2  4.5e-2    7.5e-2  1.8e-2    1.3e-1  1.4e-1
    enc_l01_fp8     6.6e-2  3.4e-2    6.1e-2  2.2e-2    1.0e-1  1.0e-1
Every gate is 2 x max(CPU emulation figure, emulation figure at size), rounded up to one digit; no gate comes from what the library's kernels
measure. The library's own figures follow the emulation closely in rel-L2 (to two or three digits) and within about 10 % in the `worst` maxima, so
a few library figures sit just above gate / 2 (up to 0.55) where the emulation sits just below it (enc_l01 update worst: emulation 9.76e-3 -> gate
2e-2, library 1.05e-2): the margin over the library is then a little under the 2x the emulation has.
With +- 100 logits softmax is an argmax over the 32 spiked keys and bf16 rounding of q / k flips it for a handful of queries: the peaky gates only
catch gross errors. What the peaky case pins sharply is that the fallback ran and recomputed everything: fallback count, bit-equality of the result
with the bf16 route, repeatability, fast against plain.
"""
import torch
import torch.nn.functional as F

from oracle import vae as ovae
from tests.golden._det import det_state_dict

CFG = dict(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2)
RES_GAIN, RES_GROWTH, QK_GAIN, V_GAIN, PEAKY_GAIN = 1.75, 1.3, 1.7, 2.0, 6.0
FP8_ACT_SCALE, FP8_MAX = 16.0, 448.0

# the segments the tests run: kind -> (half, first step name, last step name)
SEGMENTS = {
    "dec_l0": (1, "up1.us", "up0.res2"),
    "dec_l1": (1, "up2.us", "up1.res1"),
    "dec_l32": (1, "mid.res1", "up2.res0"),
    "dec_mid": (1, "mid.res0", "mid.res1"),
    "enc_l01": (0, "down0.res0", "down1.res0"),
    "enc_l23mid": (0, "down2.ds", "mid.attn"),
}

MUTATIONS = ("gn_before_residual", "stats_other_image", "cpg_halved", "no_silu_norm2", "silu_on_attn_norm", "shortcut_from_normed",
             "residual_from_conv1", "pad_before_norm", "upsample_phase_shift", "ds_pad_wrong", "no_attn_scale", "softmax_over_queries",
             "proj_res_from_normed")

METRICS = ("l2", "worst", "border_l2", "border_worst", "upd_l2", "upd_worst")
GATES = {}   # filled below


def rb(t):
    """Round to bf16, keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def steps(half):
    """[(name, kind, state-dict prefix)] of one half; kind in 'res', 'attn', 'ds', 'us'."""
    nl, nrb = len(CFG["ch_mult"]), CFG["num_res_blocks"]
    side = "decoder" if half else "encoder"
    mid = [("mid.res0", "res", f"{side}.mid_block.resnets.0"), ("mid.attn", "attn", f"{side}.mid_block.attentions.0"),
           ("mid.res1", "res", f"{side}.mid_block.resnets.1")]
    out = []
    if half:
        out += mid
        for l in range(nl - 1, -1, -1):
            i = nl - 1 - l
            out += [(f"up{l}.res{j}", "res", f"decoder.up_blocks.{i}.resnets.{j}") for j in range(nrb + 1)]
            if l:
                out.append((f"up{l}.us", "us", f"decoder.up_blocks.{i}.upsamplers.0.conv"))
    else:
        for l in range(nl):
            out += [(f"down{l}.res{j}", "res", f"encoder.down_blocks.{l}.resnets.{j}") for j in range(nrb)]
            if l != nl - 1:
                out.append((f"down{l}.ds", "ds", f"encoder.down_blocks.{l}.downsamplers.0.conv"))
        out += mid
    return out


def span(kind):
    """(half, first, count) of a named segment."""
    half, a, b = SEGMENTS[kind]
    names = [s[0] for s in steps(half)]
    return half, names.index(a), names.index(b) - names.index(a) + 1


def in_channels(sd, half, first):
    name, kind, p = steps(half)[first]
    key = {"res": p + ".norm1.weight", "attn": p + ".group_norm.weight"}.get(kind)
    return sd[key].shape[0] if key else sd[p + ".weight"].shape[1]


_W = {}


def weights(kind="base"):
    """The bf16-rounded state dict (fp32 tensors, diffusers names) of one weight set: 'base' or 'peaky'."""
    if kind not in _W:
        sd = det_state_dict(ovae.state_dict_shapes(CFG), seed=606)
        for half in (0, 1):   # the stream grows along the chain: the i-th ResnetBlock's branch grows with it
            for i, p in enumerate(p for _, kind, p in steps(half) if kind == "res"):
                for leaf in ("weight", "bias"):
                    sd[f"{p}.conv2.{leaf}"] = sd[f"{p}.conv2.{leaf}"] * (RES_GAIN * RES_GROWTH ** i)
        for k in list(sd):
            if ".to_q." in k or ".to_k." in k:
                sd[k] = sd[k] * (QK_GAIN * (PEAKY_GAIN ** 0.5 if kind == "peaky" else 1.0))
            if ".to_out.0." in k:
                sd[k] = sd[k] * V_GAIN
        _W[kind] = {k: rb(v.float()) for k, v in sd.items()}
    return _W[kind]


def input_scale(half, first):
    """The rms the stream has in front of step `first` when the chain starts from a unit-rms tensor: it grows by RES_GROWTH per ResnetBlock."""
    return RES_GROWTH ** sum(kind == "res" for _, kind, _ in steps(half)[:first])


def make_input(n, c, h, w, seed, gain=1.0, spike=False):
    """bf16-exact input [n][c][h][w] fp32: smooth + noise times `gain`, every image with a mean and a scale of its own (so that statistics of the
    wrong image show). spike: the last 32 pixels of every map are 8x as large - keys of the attention's LAST tile whose scores jump far above the
    running maximum: the fp8 d = 512 attention kernel gives such queries up and raises its flag (the peaky case's way into the fallback chain)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    yy = torch.linspace(0, 3.0, h)[:, None] + torch.linspace(0, 2.0, w)[None, :]
    x = x + 0.5 * torch.sin(yy)[None, None] * torch.randn(1, c, 1, 1, generator=g)
    scale = torch.tensor([1.0, 0.6, 1.5, 0.8])[torch.arange(n) % 4].view(n, 1, 1, 1)
    mean = torch.tensor([0.0, 0.4, -0.3, 0.2])[torch.arange(n) % 4].view(n, 1, 1, 1)
    x = (x * scale + mean) * gain
    if spike:
        x[:, :, -1, -32:] *= 8.0
    return rb(x)


class Tape:
    """GroupNorm statistics and attention k / v of a full-size pass, replayed on row bands of the same input."""

    def __init__(self):
        self.items, self.pos, self.replay = [], 0, False

    def rewind(self):
        self.pos, self.replay = 0, True

    def take(self, make):
        if self.replay:
            v = self.items[self.pos]
            self.pos += 1
            return v
        v = make()
        self.items.append(v)
        return v


class _Ctx:
    def __init__(self, sd, emulate, fp8, mutation, tape):
        self.sd, self.emulate, self.fp8, self.mut, self.tape = sd, emulate, fp8, mutation, tape
        self.pending = None   # statistics a planted bug hands to the next GroupNorm
        self.dev = {}

    def w(self, name, like):
        key = (name, like.device, like.dtype)
        if key not in self.dev:
            self.dev[key] = self.sd[name].to(like.device, like.dtype)
        return self.dev[key]

    def r(self, t):
        return rb(t) if self.emulate else t


def stats(x, groups=32):
    """(mean, var) [N][groups] in float64 (biased variance), one group at a time so that a 4-GiB tensor needs no float64 copy."""
    N, C = x.shape[:2]
    cpg = C // groups
    mean = torch.empty(N, groups, dtype=torch.float64, device=x.device)
    var = torch.empty_like(mean)
    for n in range(N):
        for g in range(groups):
            v = x[n, g * cpg:(g + 1) * cpg].double()
            var[n, g], mean[n, g] = torch.var_mean(v, unbiased=False)
    return mean, var


def _gn(c, p, x, silu, st=None, groups=32):
    """GroupNorm(32, eps 1e-6) as the per-channel scale / shift the HIP finalise leaves, then SiLU; st = statistics to use instead of x's own."""
    if st is None:
        st = c.pending if c.pending is not None else (c.tape.take(lambda: stats(x, groups)) if c.tape else stats(x, groups))
    c.pending = None
    mean, var = st
    N, C = x.shape[:2]
    cpg = C // mean.shape[1]
    rstd = (var + 1e-6).rsqrt().repeat_interleave(cpg, 1)
    gamma, beta = c.w(p + ".weight", mean), c.w(p + ".bias", mean)
    scale = (gamma[None] * rstd).to(x.dtype)[:, :, None, None]
    shift = (beta[None] - mean.repeat_interleave(cpg, 1) * gamma[None] * rstd).to(x.dtype)[:, :, None, None]
    y = x * scale + shift
    return (F.silu(y) if silu else y), (scale, shift)


def conv2d(x, w, b, stride=1, padding=0):
    """F.conv2d on the CPU; on a GPU the same sum as one matrix product per tap (plain GEMMs in x's dtype: float64 has no vendor convolution,
    and the test must not depend on which algorithm a convolution library picks)."""
    if not x.is_cuda:
        return F.conv2d(x, w, b, stride=stride, padding=padding)
    N, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    xp = (F.pad(x, (padding,) * 4) if padding else x).permute(0, 2, 3, 1)
    Ho, Wo = (H + 2 * padding - kh) // stride + 1, (W + 2 * padding - kw) // stride + 1
    out = None
    for ky in range(kh):
        for kx in range(kw):
            patch = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            t = patch.reshape(-1, C) @ w[:, :, ky, kx].T
            out = t if out is None else out.add_(t)
            del t, patch
    return out.add_(b).view(N, Ho, Wo, Co).permute(0, 3, 1, 2)


def _e4m3(t):
    return t.float().clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).to(t.dtype)


def _conv3(c, p, x, fp8=False, padding=1, stride=1):
    w, b = c.w(p + ".weight", x), c.w(p + ".bias", x)
    if fp8:   # weights.pack_conv3x3_fp8: e4m3 per output channel, scale amax / 448
        ws = (w.abs().amax(dim=(1, 2, 3), keepdim=True) / FP8_MAX).clamp_min(1e-12)
        w = _e4m3(w / ws) * ws
    return conv2d(x, w, b, stride=stride, padding=padding)


def _act(c, y, fp8):
    """How the GroupNorm + SiLU output is stored: bf16, or e4m3(y * 16)."""
    if not c.emulate:
        return y
    return _e4m3(y * FP8_ACT_SCALE) / FP8_ACT_SCALE if fp8 else rb(y)


def resnet(c, p, x):
    m = c.mut
    has_sc = p + ".conv_shortcut.weight" in c.sd
    fp8 = c.fp8 and c.emulate
    a, (scale, shift) = _gn(c, p + ".norm1", x, True)
    a = _act(c, a, fp8)
    if m == "pad_before_norm":   # the zero padding goes through norm + SiLU: border taps see silu(shift) instead of 0
        a = _act(c, F.silu(F.pad(x, (1, 1, 1, 1)) * scale + shift), fp8)
        h1 = c.r(_conv3(c, p + ".conv1", a, fp8, padding=0))
    else:
        h1 = c.r(_conv3(c, p + ".conv1", a, fp8))
    st = None
    if m == "stats_other_image" and x.shape[0] > 1:
        st = tuple(t.roll(1, 0) for t in stats(h1))
    if m == "cpg_halved":
        st = stats(h1, 64)
    b, _ = _gn(c, p + ".norm2", h1, m != "no_silu_norm2", st)
    b = _act(c, b, fp8)
    skip = x
    if has_sc:
        src = a if m == "shortcut_from_normed" else x
        skip = c.r(conv2d(src, c.w(p + ".conv_shortcut.weight", x), c.w(p + ".conv_shortcut.bias", x)))
    elif m == "residual_from_conv1":
        skip = h1
    h2 = _conv3(c, p + ".conv2", b, fp8)
    if m == "gn_before_residual":   # the epilogue's partial sums taken from the conv alone
        c.pending = stats(c.r(h2))
    return c.r(skip + h2), skip


def _softmax_pv(c, q, k, v, scale, over_queries):
    """softmax(q k^T * scale) v in float64, chunked by query blocks; emulate: P = exp(s - max) rounded to bf16, O = P v / sum(P)."""
    T = q.shape[0]
    kd, vd = k.double(), v.double()
    if over_queries:   # (small maps only)
        P = torch.softmax(q.double() @ kd.T * scale, dim=0)
        return (P @ vd).to(q.dtype)
    out = torch.empty(T, v.shape[1], dtype=q.dtype, device=q.device)
    blk = 2048
    for i in range(0, T, blk):
        s = q[i:i + blk].double() @ kd.T * scale
        s = torch.exp(s - s.amax(dim=1, keepdim=True))
        l = s.sum(dim=1, keepdim=True)
        if c.emulate:
            s = rb(s)
        out[i:i + blk] = ((s @ vd) / l).to(q.dtype)
    return out


def attn(c, p, x):
    """With a replaying tape x may be a row band: the queries are the band's, k / v those of the recorded full map."""
    m = c.mut
    N, C, H, W = x.shape
    hn, _ = _gn(c, p + ".group_norm", x, m == "silu_on_attn_norm")
    hn = c.r(hn)
    t = hn.flatten(2).transpose(1, 2)   # N, HW, C
    lin = lambda name, z: c.r(F.linear(z, c.w(f"{p}.{name}.weight", x), c.w(f"{p}.{name}.bias", x)))
    q = lin("to_q", t)
    if c.tape:
        k, v = c.tape.take(lambda: (lin("to_k", t), lin("to_v", t)))
    else:
        k, v = lin("to_k", t), lin("to_v", t)
    scale = 1.0 if m == "no_attn_scale" else C ** -0.5
    o = torch.stack([_softmax_pv(c, q[n], k[n], v[n], scale, m == "softmax_over_queries") for n in range(N)])
    o = c.r(o)
    skip = hn if m == "proj_res_from_normed" else x
    o = F.linear(o, c.w(p + ".to_out.0.weight", x), c.w(p + ".to_out.0.bias", x)).transpose(1, 2).reshape(N, C, H, W)
    return c.r(skip + o), skip


@torch.no_grad()
def segment(sd, half, first, count, x, emulate=False, fp8=False, mutation=None, tape=None):
    c = _Ctx(sd, emulate, fp8, mutation, tape)
    skip = None
    for name, kind, p in steps(half)[first:first + count]:
        if kind == "res":
            x, skip = resnet(c, p, x)
        elif kind == "attn":
            x, skip = attn(c, p, x)
        elif kind == "ds":
            pad = (1, 0, 1, 0) if mutation == "ds_pad_wrong" else (0, 1, 0, 1)
            x, skip = c.r(conv2d(F.pad(x, pad), c.w(p + ".weight", x), c.w(p + ".bias", x), stride=2)), None
        else:
            up = F.interpolate(x, scale_factor=2.0, mode="nearest")
            if mutation == "upsample_phase_shift":
                up = up.roll((1, 1), (2, 3))
            x, skip = c.r(conv2d(up, c.w(p + ".weight", x), c.w(p + ".bias", x), padding=1)), None
    return x, skip


def border(t):
    """The outermost pixel ring of [N][C][H][W], flattened."""
    return torch.cat([t[:, :, 0].flatten(), t[:, :, -1].flatten(), t[:, :, 1:-1, 0].flatten(), t[:, :, 1:-1, -1].flatten()])


def errors(got, ref, skip=None):
    """{metric: value} of `got` against `ref` (same shape, NCHW): see METRICS. The update metrics are present when skip is."""
    got, ref = got.double(), ref.double()
    d = got - ref
    rng = float(ref.max() - ref.min())
    e = dict(l2=float(d.norm() / ref.norm()), worst=float(d.abs().max()) / rng,
             border_l2=float(border(d).norm() / border(ref).norm()), border_worst=float(border(d).abs().max()) / rng)
    if skip is not None:
        upd = ref - skip.double()
        e.update(upd_l2=float(d.norm() / upd.norm()), upd_worst=float(d.abs().max() / upd.abs().max()))
    return e


def outside(e, gates):
    """The largest measured / gate ratio over the metrics present."""
    return max(e[k] / gates[k] for k in e)


def _g(*v):
    return dict(zip(METRICS, v))


GATES.update({
    "dec_l0": _g(2e-2, 8e-3, 2e-2, 4e-3, 2e-2, 3e-2),
    "dec_l1": _g(1e-2, 7e-3, 1e-2, 4e-3, 2e-2, 2e-2),
    "dec_l32": _g(2e-2, 1e-2, 2e-2, 4e-3, 3e-2, 3e-2),
    "dec_mid": _g(2e-2, 9e-3, 2e-2, 6e-3, 3e-2, 4e-2),
    "enc_l01": _g(2e-2, 7e-3, 2e-2, 5e-3, 2e-2, 2e-2),
    "enc_l23mid": _g(2e-2, 8e-3, 2e-2, 6e-3, 2e-1, 2e-1),
    "dec_mid_peaky": _g(7e-2, 4e-1, 2e-1, 4e-1, 7e-1, 7e0),
    "dec_l0_fp8": _g(2e-1, 9e-2, 2e-1, 4e-2, 3e-1, 3e-1),
    "dec_l32_fp8": _g(2e-1, 1e-1, 2e-1, 4e-2, 3e-1, 3e-1),
    "enc_l01_fp8": _g(2e-1, 9e-2, 2e-1, 6e-2, 3e-1, 3e-1),
})
