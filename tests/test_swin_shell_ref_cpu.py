"""CPU checks of the SwinIR shell reference (tests/support/swin_shell_ref.py) and of the gates tests/test_swin_shell_gpu.py applies with it.

* The restatement is the oracle: in float64, head -> oracle.swinir._block per block -> rstb_tail per RSTB -> recon equals swinir_forward to
  1e-12, at 64 x 64 and 64 x 128, at reduced width (SWIN_SMALL) and at full width with depths [1, 1].
* The seeded weights are lively: for every conv that has a skip (the two RSTB tails, conv_after_body) branch rms over skip rms lies in 0.3 .. 3,
  and every LeakyReLU sees both signs.
* The gates are derived here: R.GATES[key] = emulation (fp32 arithmetic, bf16 where the HIP path stores bf16) against float64 over the two
  CPU-sized cases, times 2, rounded up to one digit.
* Every planted bug lands at least 1.5x outside at least one gate of its part, on the case named in CASES_CPU.
"""
from functools import lru_cache

import pytest
import torch

from oracle import swinir as oswin
from tests.golden._det import det_state_dict
from tests.support import swin_shell_ref as R
from tests.support.small_models import SWIN_SMALL

CASES_CPU = {"64x64": (1, 64, 64), "64x128x2": (2, 64, 128)}
BUG_CASE = "64x128x2"   # two images, a token grid wider than it is high


def chain(sd, cfg, img, tape=None):
    """The model as the three parts with the oracle's blocks in between: (output, what every part saw and gave)."""
    n, _, h, w = img.shape
    gh, gw, C = h // 8, w // 8, cfg["embed_dim"]
    rpi = oswin._relative_position_index(8)
    x0, xa = R.head(sd, img, cfg=cfg)
    seen = dict(x0=x0, xa_head=xa, tails=[])
    for i, depth in enumerate(cfg["depths"]):
        t = xa[:, :C].reshape(n, gh * gw, C)
        for j in range(depth):
            t = oswin._block(sd, f"layers.{i}.residual_group.blocks.{j}.", t, gh, gw, cfg["num_heads"][i], 8, 0 if j % 2 == 0 else 4, rpi)
        xc = torch.nn.functional.pad(t.reshape(-1, C), (0, R.CP - C))
        out = R.rstb_tail(sd, i, xc, xa, n, gh, gw, cfg=cfg)
        seen["tails"].append((xc, xa, out))
        xa = out
    seen["xa"] = xa
    return R.recon(sd, xa, x0, n, gh, gw, cfg=cfg, tape=tape), seen


@pytest.mark.parametrize("width", ["small", "full"])
@pytest.mark.parametrize("case", list(CASES_CPU))
def test_restatement_is_the_oracle(width, case):
    n, h, w = CASES_CPU[case]
    if width == "small":
        cfg = dict(oswin.DEFAULT_CFG, **SWIN_SMALL)
        sd = det_state_dict(oswin.state_dict_shapes(cfg), seed=101)
    else:
        cfg, sd = R.CFG, R.weights()
    sd = {k: v.double() for k, v in sd.items()}
    img = R.make_image(n, h, w, seed=h + w).double()
    got, _ = chain(sd, cfg, img)
    ref = oswin.swinir_forward(sd, img, cfg)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{width} {case}: parts + oracle blocks vs swinir_forward {err:.1e}")
    assert err <= 1e-12, err


@lru_cache(maxsize=None)
def reference(case):
    """float64 chain of the full-width model on a CPU-sized case: (img, output, seen, tape)."""
    n, h, w = CASES_CPU[case]
    sd = R.weights()
    img = R.make_image(n, h, w, seed=h + w).double()
    tape = {}
    out, seen = chain({k: v.double() for k, v in sd.items()}, R.CFG, img, tape)
    return img, out, seen, tape


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


@pytest.mark.parametrize("case", list(CASES_CPU))
def test_weights_are_lively(case):
    n, h, w = CASES_CPU[case]
    img, out, seen, tape = reference(case)
    for i, (xc, xa, y) in enumerate(seen["tails"]):
        ratio = rms(y - xa) / rms(xa)
        print(f"{case} layers.{i}.conv: rms(branch) / rms(skip) = {ratio:.2f}")
        assert 0.3 <= ratio <= 3.0, (i, ratio)
    sd = {k: v.double() for k, v in R.weights().items()}
    t = R._ln(R._Ctx(sd, False, None), "norm", seen["xa"])
    branch = R._conv(R._Ctx(sd, False, None), "conv_after_body", R.to_map(t, n, h // 8, w // 8))
    ratio = rms(branch) / rms(seen["x0"][:, :R.C])
    print(f"{case} conv_after_body: rms(branch) / rms(skip) = {ratio:.2f}")
    assert 0.3 <= ratio <= 3.0, ratio
    assert set(tape) == {"before_up", "conv_up1", "conv_up2", "conv_up3", "conv_hr"}
    for name, p in tape.items():
        neg = float((p < 0).double().mean())
        print(f"{case} LeakyReLU behind {name}: {neg:.2f} of its inputs negative")
        assert 0.1 <= neg <= 0.9, (name, neg)
    # the synthetic streams the GPU test feeds are of the chain's size
    gh, gw = h // 8, w // 8
    for what, chain_t in (("xa_tail", seen["tails"][1][1]), ("xc", seen["tails"][1][0]), ("xa_recon", seen["xa"]), ("x0", seen["x0"])):
        ratio = rms(R.make_tokens(n, gh, gw, 1, gain=R.GAIN[what])[:, :R.C]) / rms(chain_t[:, :R.C])
        print(f"{case} synthetic {what}: rms {ratio:.2f} of the chain's")
        assert 0.5 <= ratio <= 2.0, (what, ratio)


def test_phase_sums_are_bf16_exact():
    """The up-conv weights sit on R.UP_GRID: the production packer's phase form (sums of taps, rounded to bf16) holds the sums themselves, so
    the 9-tap and the phase form are the same convolution and the reconstruction emulated on either agrees to rounding flips."""
    from instarevive_amd import weights as Wt
    sd = R.weights()
    groups = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    for name in ("conv_up1", "conv_up2", "conv_up3"):
        w = sd[name + ".weight"]
        assert w.unique().numel() >= 64, "the grid left too few weight levels"
        packed = Wt.pack_conv_up2x2(w).view(torch.bfloat16).float().view(4, 64, 4, 64)   # [2 dy + dx][Cout][2 sy + sx][Cin]
        for dy in (0, 1):
            for dx in (0, 1):
                for sy in (0, 1):
                    for sx in (0, 1):
                        want = sum(w[:, :, ky, kx].double() for ky in groups[dy][sy] for kx in groups[dx][sx])
                        assert torch.equal(packed[2 * dy + dx, :, 2 * sy + sx, :].double(), want), (name, dy, dx, sy, sx)
    n, h, w_ = CASES_CPU["64x64"]
    _, _, seen, _ = reference("64x64")
    xa, x0 = seen["xa"].float().double(), seen["x0"].float().double()
    a, b = (R.recon(sd, xa, x0, n, h // 8, w_ // 8, emulate=e) for e in (True, "phase"))
    diff = float((a - b).norm() / a.norm())
    print(f"reconstruction emulated on the phase form against the 9-tap form: rel-L2 {diff:.1e}")
    assert diff <= 1e-4, diff


def part_errors(case, emulate=False, mutation=None):
    """{gate key: errors} of every part on the inputs the float64 chain gave it (so that a part's error is its own)."""
    n, h, w = CASES_CPU[case]
    gh, gw = h // 8, w // 8
    sd = R.weights()
    img, out, seen, _ = reference(case)
    kw = dict(emulate=emulate, mutation=mutation)
    part = R.PLANT.get(mutation)
    e = {}
    if part in (None, "head"):
        x0, xa = R.head(sd, img, **kw)
        e["head_x0"] = R.token_errors(x0, seen["x0"], n, gh, gw)
        e["head_xa"] = R.token_errors(xa, seen["xa_head"], n, gh, gw)
    if part in (None, "rstb_tail"):
        for i, (xc, xa, y) in enumerate(seen["tails"]):
            xc, xa = R.rb(xc), xa.float().double()   # as the path holds them: bf16, fp32
            ref = R.rstb_tail(sd, i, xc, xa, n, gh, gw)
            got = R.rstb_tail(sd, i, xc, xa, n, gh, gw, x0=seen["x0"], **kw)
            ei = R.token_errors(got, ref, n, gh, gw, base=xa)
            e["rstb_tail"] = {k: max(ei[k], e.get("rstb_tail", ei)[k]) for k in ei}
    if part in (None, "recon"):
        xa, x0 = seen["xa"].float().double(), seen["x0"].float().double()
        ref = R.recon(sd, xa, x0, n, gh, gw)
        e["recon"] = R.errors(R.recon(sd, xa, x0, n, gh, gw, **kw), ref, 8)
    return e


def test_gates_are_twice_the_emulation():
    worst = {}
    for case in CASES_CPU:
        for key, e in part_errors(case, emulate=True).items():
            print(f"EMU {case} {key}: " + "  ".join(f"{m} {v:.2e}" for m, v in e.items()))
            worst[key] = {m: max(v, worst.get(key, e)[m]) for m, v in e.items()}
    for key, e in worst.items():
        derived = {m: R.round_up(2 * v) for m, v in e.items()}
        print(f"GATE {key}: " + "  ".join(f"{m} {derived[m]:.0e}" for m in e))
        for m in e:
            assert e[m] <= R.GATES[key][m] / 2, (key, m, e[m], R.GATES[key][m])
            assert abs(R.GATES[key][m] - derived[m]) <= 1e-9 * derived[m], f"GATES[{key}][{m}] is {R.GATES[key][m]:.0e}, derived {derived[m]:.0e}"


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_bugs_fail_the_gates(mutation):
    dist = {key: R.outside(e, R.GATES[key]) for key, e in part_errors(BUG_CASE, mutation=mutation).items()}
    print(f"BUG {mutation} on {BUG_CASE}: " + "  ".join(f"{k} {v:.1f}x" for k, v in dist.items()))
    assert max(dist.values()) >= 1.5, (mutation, dist)
