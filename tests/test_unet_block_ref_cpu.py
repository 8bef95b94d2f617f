"""The float64 reference of one ControlLDM UNet block (tests/support/unet_block_ref.py), on the CPU:
  * it is pinned to oracle/cldm.py (which tests/test_oracle_golden.py pins to the reference project's fixtures): every block of the
    CLDM_SMALL UNet and ControlNet against oracle.cldm._block, and the whole chain against reflow_sample, within float32 rounding;
  * the gates of tests/test_unet_block_gpu.py are derived: the reference is re-run with bf16 rounding at the HIP path's rounding points on every
    case of that test, EMULATION in the support module holds the largest error per block kind and measure, the gates are twice that;
  * every planted bug of unet_block_ref.MUTATIONS lands at least 1.5x outside a gate of its block kind: all of them do, the nearest being
    norm2 / norm3 exchanged at 9.4 x (input_blocks.8) and 15.4 x (middle_block.1), then emb_out not added at 17.8 x (input_blocks.1);
  * the whole-network gate is measured: on CLDM_SMALL with the oracle, each of the 13 control residuals is dropped in turn and the movement of
    the output printed against the 1.8 % rel-L2 gate of tests/test_cldm_gpu.py - and the gates of test_each_control_residual_alone are derived
    (the bf16 emulation of sample_log with only residual i minus sample_log without control, against the oracle's difference).
Everything is printed (run with -s)."""
import pytest
import torch

from oracle import cldm as ocldm
from tests.golden._det import det_state_dict
from tests.support import unet_block_ref as R

PLANTED_MIN = 1.5
WHOLE_NETWORK_GATE = 0.018   # tests/test_cldm_gpu.py TOL["l2"]
# mutation -> the (set, index) blocks it is planted in, on 8 x 8
PLANTED = {
    "emb_out_dropped": ((0, 10), (0, 1)), "emb_out_other_timestep": ((0, 10), (2, 0)), "shortcut_dropped": ((2, 0), (0, 4)),
    "softmax_scale_missing": ((1, 1), (0, 1)), "cross_attends_tokens": ((1, 1), (0, 5)), "geglu_halves_swapped": ((1, 1), (0, 1)),
    "norm2_norm3_swapped": ((1, 1), (0, 8)), "proj_out_residual_after_norm": ((1, 1), (0, 1)), "down_pad_0101": ((0, 3), (0, 9)),
    "up_shifted": ((2, 2), (2, 8)), "decoder_slices_swapped": ((2, 0), (2, 10), (2, 9)),
}


@pytest.fixture(scope="module")
def full():
    W = R.UNetWeights()
    return W, R.make_context(W), R.time_emb(W, R.TIMESTEP)


def small_weights():
    sd_u = det_state_dict(ocldm.state_dict_shapes(R.CLDM_SMALL), seed=R.RESIDUAL_SEEDS["unet"])
    sd_c = det_state_dict(ocldm.state_dict_shapes(R.CLDM_SMALL, control=True), seed=R.RESIDUAL_SEEDS["cnet"])
    return sd_u, sd_c


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@torch.no_grad()
def test_reference_matches_the_oracle():
    sd_u, sd_c = small_weights()
    ctx = R.residual_inputs()[2]
    t = torch.full((2,), R.TIMESTEP)
    worst = 0.0
    for control, sd in ((False, sd_u), (True, sd_c)):
        cfg = dict(R.CLDM_SMALL, control=control)
        W = R.UNetWeights(cfg, sd=sd)
        emb32 = ocldm._emb(sd, t, cfg["model_channels"])
        emb = R.time_emb(W, R.TIMESTEP)
        assert rel(emb, emb32[0]) < 1e-5
        for set_, cnt in enumerate(R.block_counts(cfg)):
            for index in range(cnt):
                cin, cout, kind, scale = R.block_io(cfg, set_, index)
                x = R.make_rows(2, 64, cin, seed=100 * set_ + index)
                got, _ = R.block(W, set_, index, x, 2, 8, 8, emb, ctx[0].double())
                x32 = R.rows_to_nchw(x, 2, 8, 8).float()
                if set_ == 1:
                    p, L = R.block_layers(cfg, set_, index)[0]
                    ref = {"res": lambda: ocldm._res(sd, p, x32, emb32), "xf": lambda: ocldm._xf(sd, p, x32, ctx.expand(2, -1, -1), cfg["num_head_channels"])}[L[0]]()
                else:
                    name = ("input_blocks", None, "output_blocks")[set_]
                    ref = ocldm._block(sd, f"{name}.{index}", [L for _, L in R.block_layers(cfg, set_, index)], x32, emb32, ctx.expand(2, -1, -1), cfg["num_head_channels"])
                e = rel(got, R.nchw_to_rows(ref))
                worst = max(worst, e)
                assert e < 1e-5, (control, set_, index, kind, e)
    print(f"\nreference vs oracle._block: worst rel-L2 over all blocks {worst:.2e}")
    zT, c_latent, _ = R.residual_inputs()
    sd = {**{"model.diffusion_model." + k: v for k, v in sd_u.items()}, **{"control_model." + k: v for k, v in sd_c.items()}}
    Wu, Wc = R.UNetWeights(R.CLDM_SMALL, sd=sd_u), R.UNetWeights(dict(R.CLDM_SMALL, control=True), sd=sd_c)
    e1 = rel(R.network(Wu, Wc, zT.double(), c_latent.double(), ctx[0].double(), 999.0), ocldm.reflow_sample(sd, zT, c_latent, ctx, R.CLDM_SMALL))
    e0 = rel(R.network(Wu, None, zT.double(), None, ctx[0].double(), 999.0), ocldm.reflow_sample(sd, zT, None, ctx, R.CLDM_SMALL))
    print(f"chained blocks vs oracle.reflow_sample: rel-L2 {e1:.2e} with control, {e0:.2e} without")
    assert e1 < 1e-5 and e0 < 1e-5


@torch.no_grad()
def test_gates_come_from_the_emulation(full):
    W, ctx, emb = full
    embe = R.time_emb(W, R.TIMESTEP, emulate=True)
    measured = {}
    print()
    for case, (set_, index, n, h, w) in R.CASES.items():
        x, cin, cout, kind, scale = R.case_inputs(W, case)
        probe = {}
        ref, base = R.block(W, set_, index, x, n, h, w, emb, ctx, probe=probe)
        emu, _ = R.block(W, set_, index, x, n, h, w, embe, ctx, emulate=True)
        assert ref.shape == (n * h * w * (scale * scale if scale > 0 else 1) // (4 if scale < 0 else 1), cout)
        e = R.errors(emu, ref, R.update_base(W, set_, index, x, base))
        print(f"EMULATION {case:24s} {kind:10s} " + " ".join("    -   " if v is None else f"{v:.2e}" for v in e)
              + (f"  self-attention logit std {probe['self_logit_std']:.2f}" if probe else ""))
        if probe:
            assert 2.0 < probe["self_logit_std"] < 4.5, (case, probe)
        assert [v is None for v in e] == [g is None for g in R.GATES[kind]], case
        assert R.inside(e, tuple(None if g is None else g / R.MARGIN for g in R.GATES[kind])), (case, e, R.GATES[kind])
        m = measured.setdefault(kind, [0.0] * 4)
        for k, v in enumerate(e):
            m[k] = max(m[k], v or 0.0)
    assert set(measured) == set(R.EMULATION)
    for kind, m in measured.items():
        rec = R.EMULATION[kind]
        print(f"GATE {kind:10s} emulation " + " ".join("    -   " if r is None else f"{v:.2e}" for v, r in zip(m, rec))
              + "  recorded " + " ".join("   -   " if r is None else f"{r:.1e}" for r in rec) + "  gate " + " ".join("   -   " if g is None else f"{g:.1e}" for g in R.GATES[kind]))
        for v, r, g in zip(m, rec, R.GATES[kind]):
            if r is not None:
                assert 0.9 * r <= v <= r, (kind, v, r)   # the recorded figure is this measurement, rounded up to two digits
                assert g == R.MARGIN * r


@torch.no_grad()
def test_planted_bugs_land_outside_the_gates(full):
    W, ctx, emb = full
    emb_other = R.time_emb(W, R.OTHER_TIMESTEP)
    assert set(PLANTED) == set(R.MUTATIONS)
    print()
    for mutation, blocks in PLANTED.items():
        for set_, index in blocks:
            cin, cout, kind, scale = R.block_io(W.cfg, set_, index)
            x = R.make_rows(1, 64, cin, seed=7 + 100 * set_ + index)
            ref, base = R.block(W, set_, index, x, 1, 8, 8, emb, ctx)
            bad, _ = R.block(W, set_, index, x, 1, 8, 8, emb, ctx, mutation=mutation, emb_other=emb_other)
            e = R.errors(bad, ref, R.update_base(W, set_, index, x, base))
            by = R.outside_by(e, R.GATES[kind])
            print(f"PLANTED {mutation:30s} in set {set_} block {index:2d} ({kind:9s}): " + " ".join("    -   " if v is None else f"{v:.2e}" for v in e) + f"  = {by:.1f} x a gate")
            assert by >= PLANTED_MIN, (mutation, set_, index, e, R.GATES[kind])


@torch.no_grad()
def test_control_residuals_dropped_and_alone():
    sd_u, sd_c = small_weights()
    zT, c_latent, ctx = R.residual_inputs()
    t = torch.full((1,), 999.0)
    control = ocldm.controlnet_forward(sd_c, zT, c_latent, t, ctx, R.CLDM_SMALL)
    assert len(control) == R.N_RESIDUALS
    full_out = zT + ocldm.unet_forward(sd_u, zT, t, ctx, control, R.CLDM_SMALL)
    bare = zT + ocldm.unet_forward(sd_u, zT, t, ctx, None, R.CLDM_SMALL)
    print()
    for i in range(R.N_RESIDUALS):
        dropped = [torch.zeros_like(c) if k == i else c for k, c in enumerate(control)]
        moved = rel(zT + ocldm.unet_forward(sd_u, zT, t, ctx, dropped, R.CLDM_SMALL), full_out)
        print(f"DROPPED residual {i:2d}: the whole output moves by rel-L2 {moved:.4f} = {moved / WHOLE_NETWORK_GATE:.2f} x the {WHOLE_NETWORK_GATE} gate")
    # each residual alone: the oracle's difference and its bf16 emulation
    Wu = R.UNetWeights(R.CLDM_SMALL, sd=R.device_weights(sd_u))
    c64 = ctx[0].double()
    emu_bare = R.network(Wu, None, zT.double(), None, c64, 999.0, emulate=True)
    for i in range(R.N_RESIDUALS):
        sd_i = R.only_residual(sd_c, i)
        only = [c if k == i else torch.zeros_like(c) for k, c in enumerate(control)]
        d_ref = (zT + ocldm.unet_forward(sd_u, zT, t, ctx, only, R.CLDM_SMALL)) - bare
        via_sd = (zT + ocldm.unet_forward(sd_u, zT, t, ctx, ocldm.controlnet_forward(sd_i, zT, c_latent, t, ctx, R.CLDM_SMALL), R.CLDM_SMALL)) - bare
        assert rel(via_sd, d_ref) < 1e-4, i   # zeroing the other zero-convs in the state dict is keeping residual i alone
        Wc = R.UNetWeights(dict(R.CLDM_SMALL, control=True), sd=R.device_weights(sd_i))
        d_emu = R.network(Wu, Wc, zT.double(), c_latent.double(), c64, 999.0, emulate=True) - emu_bare
        e = rel(d_emu, d_ref)
        print(f"ALONE residual {i:2d}: |difference| / |output| {float(d_ref.norm() / bare.norm()):.3f}, emulation rel-L2 on the difference {e:.2e}"
              f" (recorded {R.RESIDUAL_EMULATION[i]:.1e}, gate {R.RESIDUAL_GATES[i]:.1e})")
        assert e < 0.25, (i, e)   # the oracle's difference stands well above the rounding noise: residual i tests something
        assert 0.9 * R.RESIDUAL_EMULATION[i] <= e <= R.RESIDUAL_EMULATION[i], (i, e)
        assert R.RESIDUAL_GATES[i] == R.MARGIN * R.RESIDUAL_EMULATION[i]
