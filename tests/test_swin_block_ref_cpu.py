"""CPU checks of the fused-Swin-block reference (tests/support/swin_block_ref.py) and of the gates tests/test_swin_fused_gpu.py applies with it.

The restatement must be the oracle's block (oracle/swinir.py _block) when it is fed the fp32 qkv rows. The gates act on the block's UPDATE
(out - x_in: the residual stream hides a block-level bug in `out`): relative L2 <= 1e-2 and worst element <= 1e-2 of max |update|. Rounding to
bf16 where the kernels round must stay inside them with at least 2x margin, and each planted layout bug must land at least 1.5x outside.
tanh-vs-erf GELU is not among the bugs: it moves the update by about 2e-4, below bf16 noise, so no gate on the update can see it."""
import pytest
import torch

from oracle import swinir as oswin
from tests.support import swin_block_ref as R

GATE_L2, GATE_WORST = 1e-2, 1e-2
B, H, W_ = 2, 24, 40   # 15 windows per image: every window class of a shifted block occurs


@pytest.fixture(scope="module")
def wts():
    return R.BlockWeights()


@pytest.fixture(scope="module")
def shifted(wts):
    x, qkv = R.make_inputs(wts, 1, B, H, W_, seed=3)
    return x, qkv, R.block(wts, 1, qkv, x, B, H, W_, 4)


@pytest.mark.parametrize("j,shift", [(0, 0), (1, 4)])
def test_restatement_is_the_oracle_block(wts, j, shift):
    x, _ = R.make_inputs(wts, j, B, H, W_, seed=3)
    p = wts.p(j)
    ln = R.layer_norm_rows(x, wts.sd[p + "norm1.weight"], wts.sd[p + "norm1.bias"], wts.C)
    qkv32 = R.qkv_rows(ln, *wts.qkv_dev(j))
    got = R.block(wts, j, qkv32, x, B, H, W_, shift)["out"]
    ref = oswin._block(wts.sd, p, x[:, :wts.C].reshape(B, H * W_, wts.C), H, W_, R.HEADS, R.WS, shift, wts.rpi).reshape(-1, wts.C)
    assert float((got[:, :wts.C] - ref).abs().max()) <= 1e-5
    assert got[:, wts.C:].abs().max() == 0


@pytest.mark.parametrize("j,shift", [(0, 0), (1, 4)])
def test_bf16_rounding_points_stay_inside_the_gates(wts, j, shift):
    x, qkv = R.make_inputs(wts, j, B, H, W_, seed=3)
    ref = R.block(wts, j, qkv, x, B, H, W_, shift)
    emu = R.block(wts, j, qkv, x, B, H, W_, shift, emulate=True)
    for part in ("attn", "out"):
        l2, worst = R.update_error(emu[part], ref[part], x)
        print(f"bf16 emulation, shift {shift}, {part}: rel-L2 {l2:.2e}, worst {worst:.2e}")
        assert l2 <= GATE_L2 / 2 and worst <= GATE_WORST / 2, (part, l2, worst)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_layout_bugs_fail_the_gates(wts, shifted, mutation):
    x, qkv, ref = shifted
    bad = R.block(wts, 1, qkv, x, B, H, W_, 4, mutation=mutation)
    l2, worst = R.update_error(bad["out"], ref["out"], x)
    print(f"{mutation}: rel-L2 {l2:.2e}, worst {worst:.2e}")
    assert l2 >= 1.5 * GATE_L2 or worst >= 1.5 * GATE_WORST, (mutation, l2, worst)
