"""CPU checks of the VAE segment reference (tests/support/vae_segment_ref.py) and of the gates tests/test_vae_segment_gpu.py applies with it, at
full channel widths on small maps (16 x 24 for the 512-channel segments, 32 x 48 for the others).

* The restatement is the oracle: every step equals oracle.vae._resnet / _attn / the Downsample and Upsample lines, and the chain of ALL interior
  steps between the oracle's conv_in and norm_out / conv_out reproduces vae_encode_mean and vae_decode.
* The weights make lively blocks: in every ResnetBlock the branch h has an rms within 0.5x .. 2x of its skip path, the attention's logits
  have a std of at least 2 (peaky set: at least 12).
* The gates are derived here: R.GATES[kind] = bf16 (fp8) emulation error against float64, times 2, rounded up to one digit. The test asserts
  emulation <= gate / 2 and prints both.
* Every planted bug lands at least 1.5x outside at least one gate of the segment kind it is planted in. Printed: the distance of each.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import vae as ovae
from tests.support import vae_segment_ref as R

SIZES = {"dec_l0": (32, 48), "dec_l1": (32, 48), "dec_l32": (16, 24), "dec_mid": (16, 24), "enc_l01": (32, 48), "enc_l23mid": (32, 48)}
# where each bug is planted: a segment kind that contains the code it breaks
PLANT = {"gn_before_residual": "dec_l0", "stats_other_image": "dec_l0", "cpg_halved": "dec_l0", "no_silu_norm2": "dec_l0",
         "silu_on_attn_norm": "dec_mid", "shortcut_from_normed": "dec_l0", "residual_from_conv1": "dec_l0", "pad_before_norm": "dec_l0",
         "upsample_phase_shift": "dec_l0", "ds_pad_wrong": "enc_l01", "no_attn_scale": "dec_mid", "softmax_over_queries": "dec_mid",
         "proj_res_from_normed": "dec_mid"}


def setup(kind, n=2, wkind="base"):
    sd = R.weights(wkind)
    half, first, count = R.span(kind)
    h, w = SIZES[kind]
    x = R.make_input(n, R.in_channels(sd, half, first), h, w, seed=h * w + first, gain=R.input_scale(half, first), spike=wkind == "peaky").double()
    return sd, half, first, count, x


_REF = {}


def reference(kind):
    if kind not in _REF:
        sd, half, first, count, x = setup(kind)
        _REF[kind] = (x,) + R.segment(sd, half, first, count, x)
    return _REF[kind]


@pytest.mark.parametrize("half", [0, 1])
def test_restatement_is_the_oracle(half):
    """Step by step against the oracle's functions, then the whole chain against vae_encode_mean / vae_decode."""
    torch.manual_seed(half)
    sd = {k: v.double() for k, v in R.weights().items()}
    st = R.steps(half)
    if half:
        z = torch.randn(1, 4, 8, 12, dtype=torch.float64)
        x = ovae._conv(sd, "decoder.conv_in", ovae._conv(sd, "post_quant_conv", z, padding=0))
    else:
        img = torch.rand(1, 3, 32, 48, dtype=torch.float64) * 2 - 1
        x = ovae._conv(sd, "encoder.conv_in", img)
    worst = 0.0
    for i, (name, kind, p) in enumerate(st):
        got, _ = R.segment(sd, half, i, 1, x)
        if kind == "res":
            ref = ovae._resnet(sd, p, x)
        elif kind == "attn":
            ref = ovae._attn(sd, p, x)
        elif kind == "ds":
            ref = ovae._conv(sd, p, F.pad(x, (0, 1, 0, 1)), stride=2, padding=0)
        else:
            ref = ovae._conv(sd, p, F.interpolate(x, scale_factor=2.0, mode="nearest"))
        err = float((got - ref).abs().max() / ref.abs().max())
        worst = max(worst, err)
        assert err <= 1e-9, (name, err)
        x = ref
    chain, _ = R.segment(sd, half, 0, len(st), ovae._conv(sd, "decoder.conv_in", ovae._conv(sd, "post_quant_conv", z, padding=0)) if half
                         else ovae._conv(sd, "encoder.conv_in", img))
    if half:
        got = ovae._conv(sd, "decoder.conv_out", F.silu(ovae._gn(sd, "decoder.conv_norm_out", chain)))
        ref = ovae.vae_decode({k: v.float() for k, v in sd.items()}, z.float())
    else:
        got = ovae._conv(sd, "quant_conv", ovae._conv(sd, "encoder.conv_out", F.silu(ovae._gn(sd, "encoder.conv_norm_out", chain))), padding=0)[:, :4]
        ref = ovae.vae_encode_mean({k: v.float() for k, v in sd.items()}, img.float())
    err = float((got - ref.double()).abs().max() / ref.abs().max())
    print(f"half {half}: steps vs oracle worst {worst:.1e}, chain vs oracle (fp32) {err:.1e}")
    assert err <= 1e-4, err


def test_weights_make_lively_blocks():
    """h / skip rms within 0.5 .. 2 in every ResnetBlock of both halves on the way of a chain; attention logit std >= 2 (peaky >= 12)."""
    for half in (0, 1):
        sd = R.weights()
        st = R.steps(half)
        x = R.make_input(1, R.in_channels(sd, half, 0), 32 if half == 0 else 4, 48 if half == 0 else 6, seed=9).double()
        for i, (name, kind, p) in enumerate(st):
            y, skip = R.segment(sd, half, i, 1, x)
            if kind == "res":
                ratio = float((y - skip).pow(2).mean().sqrt() / skip.pow(2).mean().sqrt())
                print(f"half {half} {name}: rms(h) / rms(skip) = {ratio:.2f}")
                assert 0.5 <= ratio <= 2.0, (half, name, ratio)
            if kind == "attn":
                for wk, lo in (("base", 2.0), ("peaky", 12.0)):
                    sw = {k: v.double() for k, v in R.weights(wk).items()}
                    t = ovae._gn(sw, p + ".group_norm", x).flatten(2).transpose(1, 2)[0]
                    q, k = (F.linear(t, sw[f"{p}.to_{s}.weight"], sw[f"{p}.to_{s}.bias"]) for s in "qk")
                    std = float((q @ k.T * 512 ** -0.5).std())
                    o = R.segment(R.weights(wk), half, i, 1, x)
                    upd = float((o[0] - x).pow(2).mean().sqrt() / x.pow(2).mean().sqrt())
                    print(f"half {half} {name} ({wk}): logit std {std:.1f}, rms(update) / rms(x) = {upd:.2f}")
                    assert std >= lo, (half, wk, std)
                    assert upd >= 0.1, (half, wk, upd)
            x = y
    for seg in R.SEGMENTS:   # and in the segments as the tests feed them
        sd, half, first, count, x = setup(seg)
        for i in range(first, first + count):
            y, skip = R.segment(sd, half, i, 1, x)
            if skip is not None and R.steps(half)[i][1] == "res":
                ratio = float((y - skip).pow(2).mean().sqrt() / skip.pow(2).mean().sqrt())
                print(f"{seg} {R.steps(half)[i][0]}: rms(h) / rms(skip) = {ratio:.2f}")
                assert 0.5 <= ratio <= 2.0, (seg, i, ratio)
            x = y


def emulation(kind, wkind="base", fp8=False):
    sd, half, first, count, x = setup(kind, wkind=wkind)
    ref, skip = R.segment(sd, half, first, count, x) if wkind != "base" else reference(kind)[1:]
    emu, _ = R.segment(sd, half, first, count, x, emulate=True, fp8=fp8)
    return R.errors(emu, ref, skip)


EMULATED = [(k, "base", False) for k in R.SEGMENTS] + [("dec_mid", "peaky", False)] + [(k, "base", True) for k in ("dec_l0", "dec_l32", "enc_l01")]


@pytest.mark.parametrize("kind,wkind,fp8", EMULATED)
def test_emulation_stays_inside_half_the_gates(kind, wkind, fp8):
    gk = kind + ("_peaky" if wkind == "peaky" else "") + ("_fp8" if fp8 else "")
    e = emulation(kind, wkind, fp8)
    g = R.GATES[gk]
    print(f"EMU {gk}: " + "  ".join(f"{m} {e[m]:.2e} (gate {g[m]:.0e})" for m in e))
    for m in e:
        assert e[m] <= g[m] / 2, (gk, m, e[m], g[m])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_bugs_fail_the_gates(mutation):
    kind = PLANT[mutation]
    sd, half, first, count, _ = setup(kind)
    x, ref, skip = reference(kind)
    bad, _ = R.segment(sd, half, first, count, x, mutation=mutation)
    e = R.errors(bad, ref, skip)
    g = R.GATES[kind]
    print(f"BUG {mutation} in {kind}: " + "  ".join(f"{m} {e[m] / g[m]:.1f}x" for m in e))
    assert R.outside(e, g) >= 1.5, (mutation, e)
