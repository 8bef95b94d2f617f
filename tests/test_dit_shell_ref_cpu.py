"""CPU checks of the DiT shell reference (tests/support/dit_shell_ref.py) and of the gates tests/test_dit_shell_gpu.py applies with it.

Pins: the restatement equals oracle.dit on DIT_SMALL-sized weights, part by part (tables, embedding, final layer through a model of no layers)
and chained (with the control branch; with micro-conditioning); it reproduces the recorded dit_control_small.npz, size_embedder.npz and the
sin-cos rows of units.npz; the production position table (weights.sincos_pos_embed) equals the float64 one on a native and on three non-native
grids, within 4 x the deviation of an all-fp32 restatement of the table.
Gates: R.GATES are what this file derives (see the support module's docstring), on the very cases the GPU test runs - all of them fit a CPU.
Planted bugs: every mutation of R.MUTATIONS lands at least 1.5 x outside a gate of BUG_CASE[part]."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dit as odit
from tests.golden._det import checksum, det_input, det_state_dict
from tests.support import dit_shell_ref as R
from tests.support.small_models import DIT_SMALL

G = os.path.join(os.path.dirname(__file__), "golden")
BUG_CASE = {"tables": "micro_48x80", "embed": "embed_12x20x3", "control": "control_12x20x2", "final": "final_12x20x2"}
BUG_CASE_X0 = "x0_12x20x2"   # eps_from_channels_4_7, sqrt_acp_exchanged


def small(control=False, micro=False, layers=3):
    cfg = dict(DIT_SMALL, num_layers=layers, **(dict(copy_blocks_num=2) if control else {}), **(dict(sample_size=128, interpolation_scale=2.0) if micro else {}))
    shapes = dict(odit.state_dict_shapes(cfg), **(odit.control_state_dict_shapes(cfg, copy_blocks_num=2) if control else {}))
    return R.ShellWeights(cfg, det_state_dict(shapes, seed=404))


def chain(W, lat, c, t, y, bias, last_layers=()):
    """The whole forward from the parts: embed, (control | blocks), further base layers, final."""
    n, _, h, w = lat.shape
    gh, gw = h // 2, w // 2
    tab = R.tables(W, t, h, w)
    base_kv, copy_kv = R.prompt_kvs(W, y)
    x = R.embed(W, lat)[0]
    if c is not None:
        x = R.control(W, x, R.embed(W, c)[0], tab, (base_kv, copy_kv), bias, n, gh, gw)
    for l in (last_layers if c is not None else range(W.L)):
        x = R.DB.block(W.layer(l), x, R.block_mod(tab["modtab"][l]), base_kv[l], bias, n, gh, gw)
    return R.final(W, x, tab["fmod"], n, gh, gw)


def close(got, ref, what, tol=2e-5):
    err = float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
    print(f"{what}: worst {err:.2e}")
    assert err <= tol, (what, err)


# ------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("micro", [False, True])
def test_tables_are_the_oracle(micro):
    W = small(micro=micro, layers=2)
    sd, C = W.sd, W.C
    for t, h, w in ((400.0, 16, 24), (999.0, 24, 16)):
        emb = odit._lin(sd, "adaln_single.emb.timestep_embedder.linear_2", F.silu(odit._lin(sd, "adaln_single.emb.timestep_embedder.linear_1",
                                                                                            odit.timestep_embedding(torch.tensor([t])))))
        if micro:
            emb = emb + odit.micro_condition(sd, 1, h, w)
        t6 = odit._lin(sd, "adaln_single.linear", F.silu(emb)).view(6, C)
        tab = R.tables(W, t, h, w)
        close(tab["emb"], emb[0], f"emb t{t}")
        one = torch.tensor([0, 1, 0, 0, 1, 0.0])[:, None]
        for l in range(2):
            close(tab["modtab"][l], sd[f"transformer_blocks.{l}.scale_shift_table"] + t6 + one, f"modtab {l}")
        close(tab["fmod"], sd["scale_shift_table"] + emb + torch.tensor([[0.0], [1.0]]), "fmod")


def test_embedding_and_final_layer_are_the_oracle():
    """oracle.dit.dit_forward of a model WITHOUT layers is final(embed(.)); the embedding alone against F.conv2d + the oracle's table."""
    W = small(layers=0)
    for shape in ((1, 4, 16, 16), (2, 4, 24, 40)):
        lat = det_input(sum(shape), shape, -2, 2)
        n, _, h, w = shape
        x = R.embed(W, lat.double())[0]
        want = F.conv2d(lat, W.sd["pos_embed.proj.weight"], W.sd["pos_embed.proj.bias"], stride=2).flatten(2).transpose(1, 2)
        want = want + torch.from_numpy(odit.sincos_pos_embed(W.C, (h // 2, w // 2), W.base)).float()
        close(x, want.reshape(-1, W.C), f"embed {shape}")
        y = det_input(9, (1, 20, 64), -1, 1)
        ref = odit.dit_forward(W.sd, lat, 400.0, y, None, W.cfg)
        close(R.final(W, x, R.tables(W, 400.0, h, w)["fmod"], n, h // 2, w // 2), ref, f"final {shape}")


@pytest.mark.parametrize("variant", ["control", "micro", "plain"])
def test_chained_whole_is_the_oracle(variant):
    W = small(control=variant == "control", micro=variant == "micro")
    shape = (2, 4, 16, 24)
    lat, c = det_input(11, shape, -2, 2), det_input(12, shape, -2, 2)
    y, bias = R.make_prompts(2, 20, (13, 20), 64, seed=5)
    ref = odit.dit_forward(W.sd, lat, 400.0, y, (bias == 0).float(), W.cfg, c=c if variant == "control" else None)
    got = chain(W, lat.double(), c.double() if variant == "control" else None, 400.0, y, bias)
    close(got, ref, f"chained {variant}")
    if variant == "control":   # and the branch is no bystander
        assert float((ref - odit.dit_forward(W.sd, lat, 400.0, y, (bias == 0).float(), W.cfg)).norm() / ref.norm()) > 0.05


def test_recorded_control_fixture():
    from tests.test_oracle_golden import _dit_control_small
    fx = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(G, "dit_control_small.npz")).items() if v.dtype.kind == "f"}
    sd, dsd, cfg = _dit_control_small()
    assert abs(checksum(dsd) - float(fx["wsum_diffusers"])) < 1e-6 * float(fx["wsum_diffusers"])
    W = R.ShellWeights(cfg, dsd)
    assert (W.L, W.ncopy) == (4, 2)
    y = fx["y"].reshape(1, -1, fx["y"].shape[-1])
    got = chain(W, fx["lat"].double(), fx["c"].double(), 400.0, y, torch.zeros(1, y.shape[1]), last_layers=(3,))
    torch.testing.assert_close(got.float(), fx["out_c"], rtol=2e-4, atol=2e-5)


def test_recorded_size_embedders():
    fx = {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in np.load(os.path.join(G, "size_embedder.npz")).items()}
    S = 96
    shapes = {"mlp.0.weight": (S, 256), "mlp.0.bias": (S,), "mlp.2.weight": (S, S), "mlp.2.bias": (S,)}
    sd_c, sd_a = det_state_dict(shapes, seed=611), det_state_dict(shapes, seed=612)
    W = small(micro=True, layers=1)
    assert W.C == 3 * S
    for pre, sd in (("adaln_single.emb.resolution_embedder.", sd_c), ("adaln_single.emb.aspect_ratio_embedder.", sd_a)):
        for a, b in (("linear_1", "mlp.0"), ("linear_2", "mlp.2")):
            W.sd[pre + a + ".weight"], W.sd[pre + a + ".bias"] = sd[b + ".weight"], sd[b + ".bias"]
    like = torch.zeros((), dtype=torch.float64)
    for name, (h, w) in (("16x24", (16, 24)), ("64x64", (64, 64)), ("128x96", (128, 96))):
        add = R.tables(W, 400.0, h, w)["emb"] - R._mlp(W, "adaln_single.emb.timestep_embedder", R.sinusoid(400.0, like))
        torch.testing.assert_close(add.float(), fx["add_" + name][0], rtol=1e-5, atol=1e-6)


def pos_gate(gh, gw, base, scale):
    """POS_MARGIN x the worst deviation of the all-fp32 restatement of the table from the float64 one."""
    dev = float((R.pos_table(1152, gh, gw, base, scale, torch.float32).double() - R.pos_table(1152, gh, gw, base, scale)).abs().max())
    return R.POS_MARGIN * dev


def test_position_tables():
    from instarevive_amd import weights as Wt
    fx = np.load(os.path.join(G, "units.npz"))
    for gh, gw in ((32, 32), (32, 48)):   # the rows recorded from the reference
        tab = R.pos_table(1152, gh, gw, 32, 1.0).numpy()
        g = pos_gate(gh, gw, 32, 1.0)
        err = float(np.abs(tab[::37] - fx[f"pos_{gh}x{gw}_rows"]).max())
        print(f"units.npz {gh}x{gw}: worst {err:.2e} (gate {g:.2e})")
        assert err <= g
    for gh, gw, base, scale in ((32, 32, 32, 1.0), (12, 20, 32, 1.0), (128, 128, 32, 1.0), (100, 68, 32, 1.0), (24, 40, 64, 2.0)):
        prod = Wt.sincos_pos_embed(1152, gh, gw, base, scale)
        assert prod.dtype == torch.float32 and prod.shape == (gh * gw, 1152)
        err, g = float((prod.double() - R.pos_table(1152, gh, gw, base, scale)).abs().max()), pos_gate(gh, gw, base, scale)
        print(f"weights.sincos_pos_embed {gh}x{gw} base {base} scale {scale}: worst {err:.2e}, gate {g:.2e} ({err / g:.2f} of it)")
        assert err <= g, (gh, gw, err, g)


# ------------------------------------------------------------------------------------------------ liveliness
def test_control_terms_are_of_the_order_of_a_block_update():
    for case in R.CONTROL_CASES:
        ins = tuple(t.double() for t in R.case_inputs(case))
        tape = {}
        R.run_case(case, ins, tape=tape)
        rms = {k: float(v.pow(2).mean().sqrt()) for k, v in tape.items()}
        upd = sum(rms[f"upd{l}"] for l in range(3)) / 3
        print(f"{case}: block updates " + ", ".join(f"{rms[f'upd{l}']:.2f}" for l in range(3)) + "; " +
              ", ".join(f"{k} {rms[k]:.2f} ({rms[k] / upd:.2f} of a block update)" for k in ("before", "after0", "after1")))
        for k in ("before", "after0", "after1"):
            assert 0.5 <= rms[k] / upd <= 2.0, (k, rms[k], upd)


# ------------------------------------------------------------------------------------------------ gates
@lru_cache(maxsize=None)
def reference(case):
    ins = tuple(t.double() for t in R.case_inputs(case))
    return ins, R.run_case(case, ins)


def emulation(case):
    ins, ref = reference(case)
    if R.CASES[case][0] == "tables":   # the fp32 yardstick
        return R.measure(R.run_case(case, ins, dtype=torch.float32), ref)
    return R.measure(R.run_case(case, ins, emulate=True), ref)


def test_gates_are_derived_from_the_emulation():
    worst = {}
    for case in R.CASES:
        for key, e in emulation(case).items():
            print(f"EMU {case} {key}: rel-L2 {e[0]:.2e}  worst {e[1]:.2e}")
            w = worst.get(key, (0.0, 0.0))
            worst[key] = (max(w[0], e[0]), max(w[1], e[1]))
    assert set(worst) == set(R.GATES)
    for key, e in worst.items():
        margin = R.TABLES_MARGIN if key.startswith("tables_") else R.MARGIN
        derived = tuple(R.round_up(margin * v) for v in e)
        print(f"GATE {key}: rel-L2 {derived[0]:.0e}  worst {derived[1]:.0e}   (largest figure {e[0]:.2e} / {e[1]:.2e}, margin {margin:.0f} x)")
        for v, g, d in zip(e, R.GATES[key], derived):
            assert abs(g - d) <= 1e-9 * d, f"GATES[{key}] holds {g:.0e}, derived {d:.0e}"
            assert margin * v <= g


# ------------------------------------------------------------------------------------------------ planted bugs
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_planted_bugs_fail_the_gates(mutation):
    case = BUG_CASE_X0 if mutation in ("eps_from_channels_4_7", "sqrt_acp_exchanged") else BUG_CASE[R.PLANT[mutation]]
    ins, ref = reference(case)
    e = R.measure(R.run_case(case, ins, mutation=mutation), ref)
    g = R.gates_of(case)
    dist = {k: R.outside(e[k], g[k]) for k in e}
    print(f"BUG {mutation} on {case}: " + "  ".join(f"{k} {v:.3g}x" for k, v in dist.items()))
    assert max(dist.values()) >= 1.5, (mutation, dist)
