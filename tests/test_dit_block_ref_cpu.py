"""CPU checks of the DiT block reference (tests/support/dit_block_ref.py) and of the gates tests/test_dit_block_gpu.py applies with it, at full width
on a 16 x 24 token grid (384 tokens per item).

The restatement must be the oracle's block: fed the oracle's patch embedding and followed by its final layer, it reproduces
oracle.dit.dit_forward of the one-layer model. The gates act on the block's UPDATE (x_out - x_in): relative L2 <= 1e-2 and worst element <= 1e-2
of max |update| (peaky scores: 4e-2 / 8e-2). Rounding to bf16 where the HIP path rounds must stay inside them with at least 2x margin (about
3.3e-3 / 3.4e-3; peaky 1.5e-2 / 2.6e-2), and each planted bug must land at least 1.5x outside. The bugs are planted on two items with two prompts of 25 and 40 real tokens whose padding carries
diffusers' -10000 bias. One bug the gates cannot see: under the reference CLI's mask form (+1 on real tokens, 0 on padding, added as is), masking
the last real token moves that token's logit by -1 only, and the update by about 3e-3 - inside bf16 noise."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dit as odit
from tests.support import dit_block_ref as R

GATE_L2, GATE_WORST = R.GATES["base"]
GH, GW = 16, 24
T = GH * GW


@pytest.fixture(scope="module")
def base():
    return R.DitWeights()


@pytest.fixture(scope="module")
def branches():
    return R.DitWeights(qk_norm=True, kv_compress=True)


def setup(W, n, P, valid, form, seed=3):
    y, bias = R.make_prompts(P, 300, valid, seed=11, form=form)
    x = R.make_tokens(n, T, seed)
    return x, y, bias, R.modulation(W, 400.0), R.prompt_kv(W, y)


def restated_forward(W, lat, y, bias, n):
    """dit_forward of the one-layer model with the block replaced by the restatement: the oracle's patch embedding + position table in front,
    its final layer (scale_shift_table + embedded timestep, LayerNorm, proj_out, unpatchify) behind."""
    sd = {k: v.double() for k, v in W.sd.items()}
    x = F.conv2d(lat.double(), sd["pos_embed.proj.weight"], sd["pos_embed.proj.bias"], stride=2).flatten(2).transpose(1, 2)
    x = (x + torch.from_numpy(odit.sincos_pos_embed(R.C, (GH, GW), 32)).float().double()).reshape(n * T, R.C)
    x = R.block(W, x, R.modulation(W, 400.0), R.prompt_kv(W, y), bias, n, GH, GW).view(n, T, R.C)
    emb = W.lin("adaln_single.emb.timestep_embedder.linear_2", F.silu(W.lin("adaln_single.emb.timestep_embedder.linear_1", R.timestep_embedding(400.0))))
    shift, scale = (sd["scale_shift_table"][None] + emb[:, None]).chunk(2, dim=1)
    x = W.lin("proj_out", F.layer_norm(x, (R.C,), eps=1e-6) * (1 + scale) + shift).reshape(n, GH, GW, 2, 2, 8)
    return torch.einsum("nhwpqc->nchpwq", x).reshape(n, 8, 2 * GH, 2 * GW)


@pytest.mark.parametrize("variant", ["base", "qknorm_kvc"])
def test_restatement_is_the_oracle_block(base, branches, variant):
    W, n, form = (base, 2, "2d") if variant == "base" else (branches, 1, "cli")
    y, bias = R.make_prompts(n, 300, (25, 40)[:n], seed=11, form=form)
    mask = (bias == 0).float() if form == "2d" else bias[:, None]
    lat = torch.randn(n, 4, 2 * GH, 2 * GW, generator=torch.Generator().manual_seed(5))
    ref = odit.dit_forward(W.sd, lat, 400.0, y, mask, W.cfg).double()
    got = restated_forward(W, lat, y, bias, n)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{variant}: restatement vs oracle, worst {err:.2e}")
    assert err <= 1e-5, err


def test_weights_make_a_lively_block(base):
    """Self-attention logits have a std of about 3 (no flat softmax), and each of the three branches moves the update visibly: removing its
    output projection changes the update by more than 20 %."""
    x, y, bias, mod, kv = setup(base, 1, 1, (25,), "cli")
    h = F.layer_norm(x, (R.C,), eps=1e-6) * (1 + mod[1]) + mod[0]
    q, k = (base.lin(R.P_ + f"attn1.to_{s}", h).view(T, R.HEADS, R.HD).transpose(0, 1) for s in "qk")
    std = float(((q @ k.transpose(-1, -2)) * R.HD ** -0.5).std())
    print(f"self-attention logit std {std:.2f}")
    assert 2.5 <= std <= 3.5, std
    ref = R.block(base, x, mod, kv, bias, 1, GH, GW)
    for branch in ("attn1.to_out.0", "attn2.to_out.0", "ff.net.2"):
        W = R.DitWeights()
        for leaf in ("weight", "bias"):
            W.sd[R.P_ + branch + "." + leaf] = torch.zeros_like(W.sd[R.P_ + branch + "." + leaf])
        l2, _ = R.update_error(R.block(W, x, mod, kv, bias, 1, GH, GW), ref, x)
        print(f"without {branch}: the update moves by {l2:.2f}")
        assert l2 >= 0.2, (branch, l2)


@pytest.mark.parametrize("variant", ["base", "qknorm_kvc", "peaky"])
def test_bf16_rounding_points_stay_inside_the_gates(base, branches, variant):
    W, n, P, valid, form = dict(base=(base, 2, 2, (25, 40), "2d"), qknorm_kvc=(branches, 1, 1, (25,), "cli"),
                                peaky=(R.DitWeights(q_gain=R.PEAKY_GAIN * R.Q_GAIN), 1, 1, (25,), "cli"))[variant]
    g_l2, g_worst = R.GATES["peaky" if variant == "peaky" else "base"]
    x, y, bias, mod, kv = setup(W, n, P, valid, form)
    ref = R.block(W, x, mod, kv, bias, n, GH, GW)
    emu = R.block(W, x, mod, R.prompt_kv(W, y, emulate=True), bias, n, GH, GW, emulate=True)
    l2, worst = R.update_error(emu, ref, x)
    print(f"bf16 emulation, {variant}: rel-L2 {l2:.2e}, worst {worst:.2e}")
    assert l2 <= g_l2 / 2 and worst <= g_worst / 2, (l2, worst)


@pytest.fixture(scope="module")
def two_prompts(base):
    x, y, bias, mod, kv = setup(base, 2, 2, (25, 40), "2d")
    return x, bias, mod, kv, R.block(base, x, mod, kv, bias, 2, GH, GW)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_bugs_fail_the_gates(base, two_prompts, mutation):
    x, bias, mod, kv, ref = two_prompts
    bad = R.block(base, x, mod, kv, bias, 2, GH, GW, mutation=mutation)
    l2, worst = R.update_error(bad, ref, x)
    print(f"{mutation}: rel-L2 {l2:.2e}, worst {worst:.2e}")
    assert l2 >= 1.5 * GATE_L2 or worst >= 1.5 * GATE_WORST, (mutation, l2, worst)
