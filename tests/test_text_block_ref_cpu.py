"""CPU side of the text-encoder block tests: tests/support/text_block_ref.py (the float64 reference of tests/test_text_block_gpu.py) is pinned, its
gates are derived, and planted bugs are shown to land outside them.

    * the chain EMBED -> (ATTN, FFN) x L -> FINAL equals oracle.t5.t5_encode / oracle.clip_text.encode_with_transformer in float64 to 1e-12
    * the reference reproduces the third-party pins of tests/golden/text_pins.npz (transformers' buckets, T5EncoderModel at 300 tokens and with a
      fully masked item, CLIPTextModel "last" / "penultimate")
    * GATES / CASE_GATES are what the rule gives: 2 x the error of the float64 emulation that rounds where the HIP path stores bf16 (8 x the fp32
      evaluation for the fp32 parts), the largest over the cases, rounded up to one digit - no figure of the HIP kernels enters
    * every planted bug of R.PLANT lands at least 1.5 x outside a gate of its named case; those no bf16 gate can see (R.INVISIBLE) stay listed with
      their measured effect"""
from functools import lru_cache
import os

import numpy as np
import pytest
import torch

from tests.golden import make_text_pins as P
from tests.golden._det import checksum
from tests.support import text_block_ref as R

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_pins.npz")
LAND = 1.5


def ins64(case):
    ids, x, mask = R.case_inputs(case)
    return ids, None if x is None else x.double(), mask


@lru_cache(maxsize=None)
def emulation():
    """{case: {gate key: (rel-L2, worst)}} of the bf16 emulation (fp32 for the fp32 parts) against the float64 reference, and the references."""
    out, refs = {}, {}
    with torch.no_grad():
        for case, c in R.CASES.items():
            ins = ins64(case)
            ref, emu = R.run_case(case, ins), R.run_case(case, ins, emulate=True)
            e = R.measure(case, emu, ref)
            if c[0] == "attn":   # the attention output alone, against a float64 softmax over the emulation's own bf16 q|k|v
                a64 = R.att_from_qkv(R.weights(c[1]), emu["qkv"], c[3], c[4], ins[2])
                e[R.prefix(case) + "att"] = R.errors(R.rb(a64), a64)
            out[case] = e
            refs[case] = {k: v for k, v in ref.items() if c[1] != "xxl1"}
            if c[1] == "xxl1" and case == [k for k, v in R.CASES.items() if v[1] == "xxl1"][-1]:
                R.drop_weights("xxl1")
    return out, refs


@pytest.mark.parametrize("name,B,T,valid", [("narrow64", 2, 40, (40, 7)), ("narrow32", 3, 24, (24, 0, 11)), ("narrow32", 1, 300, None)])
def test_t5_chain_equals_the_oracle(name, B, T, valid):
    from oracle import t5 as ot5
    W = R.weights(name)
    ids, mask = R.make_ids(B, T, W.vocab, 11), R.make_mask(B, T, valid)
    want = ot5.t5_encode(W.sd64(), ids, mask, W.cfg).reshape(B * T, W.D)
    got = R.chain(W, ids, mask)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name,B", [("clip2", 1), ("clip4", 3), ("vith1", 2)])
def test_clip_chain_equals_the_oracle(name, B):
    from oracle import clip_text as oclip
    W = R.weights(name)
    ids = R.make_ids(B, 77, W.vocab, 12)
    want = oclip.encode_with_transformer(W.sd64(), ids, W.cfg).reshape(B * 77, W.D)
    got = R.chain(W, ids)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_buckets_reproduce_transformers():
    """(a): the reference's integer rule gives transformers' bucket for every rel = -511 .. 511, and its bias tables follow it."""
    pin = torch.from_numpy(np.load(PINS)["bucket"].astype(np.int64))
    assert torch.equal(R.bucket_table(), pin)
    assert sorted(set(pin.tolist())) == [b for b in range(32) if b != 16]   # every bucket that can occur (16 = "0 to the right" cannot), the far ones included
    W = R.weights("narrow64")
    like = torch.zeros((), dtype=torch.float64)
    for T in (1, 8, 9, 128, 129, 300, 512):
        pos = torch.arange(T)
        want = W.w(R.REL, like)[pin[(pos[None, :] - pos[:, None]) + 511]].permute(2, 0, 1)
        assert torch.equal(R.t5_bias(W, T, like), want), T
    assert not torch.equal(R.bucket_table(mutation="far_bucket"), pin) and not torch.equal(R.bucket_table(mutation="log_base"), pin)


class PinnedT5(R.TextWeights):
    def __init__(self):   # the pins' model: T5_SMALL with the fixture's seeded weights
        from oracle import t5 as o
        c = P.T5_SMALL
        self.name, self.which, self.q_gain, self.cfg = "pin_t5", R.T5, 1.0, dict(o.DEFAULT_CFG, **c)
        self.D, self.H, self.dk, self.F, self.L, self.vocab = c["d_model"], c["num_heads"], c["d_kv"], c["d_ff"], c["num_layers"], c["vocab_size"]
        self.sd, self._dev = P.t5_small_sd(), {}


class PinnedClip(R.TextWeights):
    def __init__(self, layer):
        from oracle import clip_text as o
        c = P.CLIP_SMALL
        sd = P.clip_small_sd()
        self.name, self.which, self.q_gain, self.cfg = "pin_clip", R.CLIP, 1.0, dict(o.DEFAULT_CFG, **c)
        self.D, self.H, self.vocab, self.T = c["width"], c["heads"], c["vocab_size"], c["context_length"]
        self.L = c["layers"] - (1 if layer == "penultimate" else 0)
        self.dk, self.F, self.sd, self._dev = self.D // self.H, 4 * self.D, sd, {}


def test_reference_reproduces_the_transformers_pins():
    """(b) - (d) at test_oracle_golden.py's rtol = 2e-4, atol = 2e-5; the fully masked item's rows are finite and equal transformers'."""
    fx = np.load(PINS)
    W = PinnedT5()
    assert abs(checksum(W.sd) - float(fx["t5_wsum"])) < 1e-6 * float(fx["t5_wsum"])
    for tag in ("long", "full"):
        ids, mask = torch.from_numpy(fx[f"t5_{tag}_ids"].astype(np.int64)), torch.from_numpy(fx[f"t5_{tag}_mask"].astype(np.float32))
        got = R.chain(W, ids, mask).reshape(*ids.shape, W.D)
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got.float(), torch.from_numpy(fx[f"t5_{tag}_out"]), rtol=2e-4, atol=2e-5)
    ids = torch.from_numpy(fx["clip_ids"].astype(np.int64))
    for layer in ("last", "penultimate"):
        W = PinnedClip(layer)
        assert abs(checksum(W.sd) - float(fx["clip_wsum"])) < 1e-6 * float(fx["clip_wsum"])
        torch.testing.assert_close(R.chain(W, ids).reshape(2, 77, W.D).float(), torch.from_numpy(fx["clip_" + layer]), rtol=2e-4, atol=2e-5)


def test_gates_are_derived_from_the_emulation():
    emu, _ = emulation()
    common = [c for c in emu if c not in R.OWN_GATES]

    def rule(cases, key):
        m = R.FP32_MARGIN if key in R.FP32_KEYS else R.MARGIN
        return tuple(R.round_up(m * max(emu[c][key][i] for c in cases if key in emu[c])) for i in (0, 1))

    keys = sorted({k for c in common for k in emu[c]})
    assert sorted(R.GATES) == keys
    for k in keys:
        print(f"GATE {k}: {rule(common, k)} recorded {R.GATES[k]}; emulation " + ", ".join(f"{c} {emu[c][k][0]:.2e} / {emu[c][k][1]:.2e}" for c in common if k in emu[c]))
        assert R.GATES[k] == pytest.approx(rule(common, k), rel=1e-9, abs=0), k
    assert sorted(R.CASE_GATES) == sorted(R.OWN_GATES)
    for c in R.OWN_GATES:
        own = {k: rule([c], k) for k in emu[c] if not k.endswith("_att")}
        print(f"GATE of {c}: {own} recorded {R.CASE_GATES[c]}")
        assert sorted(own) == sorted(R.CASE_GATES[c])
        for k, g in own.items():
            assert R.CASE_GATES[c][k] == pytest.approx(g, rel=1e-9, abs=0), (c, k)
            assert g[0] > R.GATES[k][0] or g[1] > R.GATES[k][1], f"{c} needs no gate of its own for {k}"
    assert R.GATES["t5_embed"] == (0.0, 0.0)   # a bf16 row widened to fp32 is exact
    for c in emu:   # what the GPU test re-measures stays under half of every gate (an eighth for the fp32 parts)
        for k, g in R.gates_of(c).items():
            assert emu[c][k][0] <= g[0] / 2 and emu[c][k][1] <= g[1] / 2, (c, k)


def test_the_cases_are_what_their_names_say():
    W = R.weights("peaky64")
    _, x, mask = ins64("t5_peaky")
    spread = R.logit_spread(W, x, 2, 120, mask)
    flat = R.logit_spread(R.weights("narrow32"), ins64("t5_t120x2")[1], 2, 120, ins64("t5_t120x2")[2])
    print(f"median logit spread: peaky {spread:.1f}, t120x2 {flat:.1f}")
    assert 27.0 <= spread <= 33.0 and flat < 15.0
    x = R.make_stream(77, 256, 1, "outlier")
    big = x.abs().amax(0) > 50
    assert 1 <= int(big.sum()) <= 3   # 1 % of 256 channels
    # distances >= 128 reach valid keys at 300 tokens with 170 valid ones, and not at the 40 tokens of the older fixture
    assert int(R.make_mask(2, 300, (300, 170))[1].sum()) > 128
    m = R.make_mask(3, 24, (24, 0, 11))
    assert float(m[1].sum()) == 0 and float(m[0].sum()) == 24
    # a fully masked item attends uniformly to all T keys: the mean of v
    q = torch.randn(1, 2, 5, 4, dtype=torch.float64)
    v = torch.randn(1, 2, 5, 4, dtype=torch.float64)
    out = R.attention(q, q, v, torch.randn(2, 5, 5, dtype=torch.float64), torch.zeros(1, 5))
    assert torch.allclose(out, v.mean(2, keepdim=True).expand_as(v), atol=1e-14)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_bug_lands_outside_a_gate(mutation):
    part, case = R.PLANT[mutation]
    assert R.CASES[case][0] == part
    _, refs = emulation()
    with torch.no_grad():
        bad = R.run_case(case, ins64(case), mutation=mutation)
    e, g = R.measure(case, bad, refs[case]), R.gates_of(case)
    worst = max(R.outside(e[k], g[k]) if g[k][0] > 0 else float("inf") for k in e)
    print(f"PLANTED {mutation} on {case}: " + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in e.items()) + f" -> {worst:.2f} x a gate")
    if mutation in R.INVISIBLE:   # recorded, not dropped: no bf16 gate can see it
        assert worst < 1.0 and worst == pytest.approx(R.INVISIBLE[mutation], rel=0.25), worst
    else:
        assert worst >= LAND, f"{mutation}: only {worst:.2f} x a gate of {case}"
