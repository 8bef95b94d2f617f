"""ControlLDM one-step path on the GPU: instarevive_amd.cldm (HIP kernels through the C ABI) against the fixtures the
reference's own ControlledUnetModel / ControlNet / Reflow_ControlLDM produced (tests/golden/cldm_small.npz, diffusion/cldm.py:32-292,
486-490,568-588) and against oracle/cldm.py (pinned to the same fixtures by tests/test_oracle_golden.py).

Tolerances: activations are bf16 between kernels (2^-9 relative) through ~25 ResBlocks and 16 transformer blocks per network; measured
rel-L2 is printed, the gates are UNet / ControlNet + UNet <= 1.8 % relative L2 [measured 0.5-1.3 %] and worst element <= 2 % of the output range; the memory-bound
kernels (GroupNorm, GEGLU) are compared with PyTorch fp32 on the same bf16-rounded data to bf16 output rounding (<= 1 bf16 ulp + 1e-3).
Below the whole network: test_each_control_residual_alone here (one of the 13 control residuals at a time, gated on the difference it makes)
and tests/test_unet_block_gpu.py (one full-width block at a time)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cldm as ocldm
from oracle import swinir as oswin
from oracle import vae as ovae
from tests.golden._det import det_input, det_state_dict

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = dict(l2=0.018, worst=0.02)
CLDM_SMALL = dict(model_channels=64, channel_mult=(1, 2, 4, 4), num_res_blocks=2, attention_resolutions=(4, 2, 1), num_head_channels=32,
                  context_dim=64, in_channels=4, hint_channels=4, out_channels=4)
SWIN_SMALL = dict(embed_dim=60, depths=[2, 2], num_heads=[6, 6])


def load(name):
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in np.load(os.path.join(G, name)).items()}


def check(got, ref, what, l2=TOL["l2"], worst=TOL["worst"]):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    r = float((got - ref).norm() / ref.norm())
    w = float((got - ref).abs().max() / (ref.max() - ref.min()))
    print(f"{what}: rel-L2 {r:.4f}, worst/range {w:.4f}")
    assert r <= l2 and w <= worst, f"{what}: rel-L2 {r:.4f} (<= {l2}), worst/range {w:.4f} (<= {worst})"


def bf16_bits(t):
    return t.to(torch.bfloat16).contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n,h,w,ch,eps,silu", [(1, 64, 64, 320, 1e-5, 1), (2, 33, 17, 640, 1e-6, 0), (1, 32, 32, 960, 1e-5, 1), (1, 16, 16, 1280, 1e-5, 1),
                                               (1, 40, 24, 1920, 1e-5, 1), (1, 8, 8, 2560, 1e-5, 1), (2, 16, 16, 64, 1e-6, 0), (1, 96, 96, 320, 1e-5, 1)])
def test_groupnorm_any(ctx, n, h, w, ch, eps, silu):
    """GroupNorm32 + optional SiLU over the UNet's channel counts (10 ... 80 channels per group) vs PyTorch fp32 on the same bf16 data."""
    torch.manual_seed(ch + h)
    x = (torch.randn(n, h * w, ch) * 1.7 + 0.3).to(torch.bfloat16)
    g, b = torch.rand(ch) + 0.5, torch.randn(ch) * 0.2
    ref = F.group_norm(x.float().transpose(1, 2).reshape(n, ch, h, w), 32, g, b, eps)
    ref = (F.silu(ref) if silu else ref).reshape(n, ch, h * w).transpose(1, 2)
    xd, gd, bd = x.cuda(), g.cuda(), b.cuda()
    y = torch.empty_like(xd)
    ws = torch.empty(n * 32 * 64 * 2 + 2 * n * ch + 64, dtype=torch.float32, device="cuda")
    rc = ctx.lib.ir_op_groupnorm_any(ctx.h, ctx.stream(), xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), n, h * w, ch, 32, eps, silu,
                                     ws.data_ptr(), ws.numel() * 4)
    ctx.check(rc, "ir_op_groupnorm_any")
    torch.cuda.synchronize()
    err = (y.float().cpu() - ref).abs()
    tol = ref.abs() * 2.0 ** -7 + 2e-3
    assert bool((err <= tol).all()), f"max err {float(err.max()):.4g} at |ref| {float(ref.abs().flatten()[err.argmax()]):.3g}"


def test_geglu(ctx):
    torch.manual_seed(3)
    rows, f = 1000, 1280
    ag = (torch.randn(rows, 2 * f) * 2).to(torch.bfloat16)
    ref = ag[:, :f].float() * F.gelu(ag[:, f:].float())
    agd = ag.cuda()
    out = torch.empty(rows, f, dtype=torch.bfloat16, device="cuda")
    ctx.check(ctx.lib.ir_op_geglu(ctx.h, ctx.stream(), agd.data_ptr(), out.data_ptr(), rows, f), "ir_op_geglu")
    torch.cuda.synchronize()
    err = (out.float().cpu() - ref).abs()
    assert bool((err <= ref.abs() * 2.0 ** -7 + 1e-3).all()), float(err.max())


# ---------------------------------------------------------------------------------------------- networks
def make_cldm(cfg=CLDM_SMALL, vae_ch=32, swin_cfg=SWIN_SMALL, seeds=(707, 708, 202, 101), clip=None):
    """A Reflow_ControlLDM with deterministic weights, loaded through the reference's checkpoint layout."""
    from instarevive_amd.cldm import Reflow_ControlLDM
    sd_u = det_state_dict(ocldm.state_dict_shapes(cfg), seed=seeds[0])
    sd_c = det_state_dict(ocldm.state_dict_shapes(cfg, control=True), seed=seeds[1])
    sd_v = det_state_dict(ovae.state_dict_shapes(dict(ch=vae_ch)), seed=seeds[2])
    sd_s = det_state_dict(oswin.state_dict_shapes(swin_cfg), seed=seeds[3])
    unet_params = dict(image_size=32, in_channels=4, out_channels=4, model_channels=cfg["model_channels"], attention_resolutions=[4, 2, 1], num_res_blocks=2,
                       channel_mult=list(cfg["channel_mult"]), num_head_channels=cfg["num_head_channels"], use_spatial_transformer=True,
                       use_linear_in_transformer=True, transformer_depth=1, context_dim=cfg["context_dim"], use_checkpoint=True, legacy=False)
    ctrl_params = dict(unet_params, hint_channels=4)
    ctrl_params.pop("out_channels")
    fs = dict(ddconfig=dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=vae_ch, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
                            attn_resolutions=[], dropout=0.0))
    full = dict(oswin.DEFAULT_CFG, **swin_cfg)
    pp = dict(img_size=64, patch_size=1, in_chans=3, embed_dim=full["embed_dim"], depths=full["depths"], num_heads=full["num_heads"], window_size=8,
              mlp_ratio=full["mlp_ratio"], sf=8, img_range=1.0, upsampler="nearest+conv", resi_connection="1conv", unshuffle=True, unshuffle_scale=8)
    m = Reflow_ControlLDM(control_stage_config=dict(target="diffusion.cldm.ControlNet", params=ctrl_params),
                          unet_config=dict(target="diffusion.cldm.ControlledUnetModel", params=unet_params),
                          first_stage_config=dict(target="ldm.models.autoencoder.AutoencoderKL", params=fs),
                          preprocess_config=dict(target="diffusion.model.swinir.SwinIR", params=pp), control_key="hint", sd_locked=False,
                          only_mid_control=False, learning_rate=1e-5, lora_rank=4, timesteps=1000, scale_factor=0.18215,
                          cond_stage_config=None if clip is None else dict(target="ldm.modules.encoders.modules.FrozenOpenCLIPEmbedder",
                                                                            params=dict(freeze=True, layer="penultimate", **clip[0])))
    # the reference's checkpoint layout: LDM names for both VAE halves (diffusers -> LDM is the inverse of weights.vae_ldm_to_diffusers)
    ldm_v = diffusers_to_ldm(sd_v)
    ckpt = {**{"model.diffusion_model." + k: v for k, v in sd_u.items()}, **{"control_model." + k: v for k, v in sd_c.items()},
            **{"cond_encoder." + k: v for k, v in ldm_v.items() if k.startswith(("encoder.", "quant_conv."))},
            **{"first_stage_model." + k: v for k, v in ldm_v.items()},
            **{"preprocess_model." + k: v for k, v in sd_s.items()},
            "betas": torch.zeros(1000)}
    if clip is not None:
        ckpt.update({"cond_stage_model.model." + k: v for k, v in clip[1].items()})
    m.load_state_dict(ckpt, strict=False)
    return m.to("cuda"), dict(unet=sd_u, cnet=sd_c, vae=sd_v, swin=sd_s)


def diffusers_to_ldm(sd, nl=4, nrb=2):
    out = {}
    res = (("norm1", "norm1"), ("conv1", "conv1"), ("norm2", "norm2"), ("conv2", "conv2"), ("conv_shortcut", "nin_shortcut"))

    def mv(src, dst, conv1x1=False):
        for t in ("weight", "bias"):
            if f"{src}.{t}" in sd:
                v = sd[f"{src}.{t}"]
                out[f"{dst}.{t}"] = v.reshape(*v.shape, 1, 1) if conv1x1 and t == "weight" and v.dim() == 2 else v

    for half in ("encoder", "decoder"):
        mv(f"{half}.conv_in", f"{half}.conv_in"); mv(f"{half}.conv_out", f"{half}.conv_out"); mv(f"{half}.conv_norm_out", f"{half}.norm_out")
        for i, b in ((0, "block_1"), (1, "block_2")):
            for a, c in res:
                mv(f"{half}.mid_block.resnets.{i}.{a}", f"{half}.mid.{b}.{c}")
        for a, c in (("group_norm", "norm"), ("to_q", "q"), ("to_k", "k"), ("to_v", "v"), ("to_out.0", "proj_out")):
            mv(f"{half}.mid_block.attentions.0.{a}", f"{half}.mid.attn_1.{c}", conv1x1=True)
        for l in range(nl):
            if half == "encoder":
                for j in range(nrb):
                    for a, c in res:
                        mv(f"encoder.down_blocks.{l}.resnets.{j}.{a}", f"encoder.down.{l}.block.{j}.{c}")
                mv(f"encoder.down_blocks.{l}.downsamplers.0.conv", f"encoder.down.{l}.downsample.conv")
            else:
                i = nl - 1 - l
                for j in range(nrb + 1):
                    for a, c in res:
                        mv(f"decoder.up_blocks.{i}.resnets.{j}.{a}", f"decoder.up.{l}.block.{j}.{c}")
                mv(f"decoder.up_blocks.{i}.upsamplers.0.conv", f"decoder.up.{l}.upsample.conv")
    mv("quant_conv", "quant_conv"); mv("post_quant_conv", "post_quant_conv")
    return out


@pytest.fixture(scope="module")
def small():
    return make_cldm()


def test_unet_alone_vs_reference_fixture(small):
    m, _ = small
    fx = load("cldm_small.npz")
    ctx_t = fx["context"].expand(fx["x"].shape[0], -1, -1).contiguous()
    out = m.model.diffusion_model(fx["x"], timesteps=torch.full((2,), 999.0), context=ctx_t, control=None)
    check(out, fx["unet_alone"], "UNet alone vs reference")


def test_sample_log_vs_reference_fixture(small):
    """Reflow_ControlLDM.sample_log with the ControlNet (13 control residuals) and without, on the reference's own outputs."""
    m, _ = small
    fx = load("cldm_small.npz")
    B = fx["zT"].shape[0]
    ctx_t = fx["context"].expand(B, -1, -1).contiguous()
    cond = {"c_concat": [torch.zeros(B, 3, 128, 128)], "c_crossattn": [ctx_t], "c_latent": [fx["c_latent"]]}
    out = m.sample_log(cond, steps=1, zT=fx["zT"])
    check(out, fx["sample"], "sample_log (ControlNet + UNet) vs reference")
    eps = m.apply_model(fx["x"], torch.full((B,), 999.0), dict(cond, c_latent=[fx["c_latent"]]))
    check(eps, fx["unet_controlled"], "apply_model vs reference")
    cond["c_latent"] = None
    check(m.sample_log(cond, steps=1, zT=fx["zT"]), fx["sample_no_control"], "sample_log without control vs reference")
    # batch rows are independent: row 1 alone gives the same result
    cond1 = {"c_concat": [torch.zeros(1, 3, 128, 128)], "c_crossattn": [ctx_t[:1].contiguous()], "c_latent": [fx["c_latent"][1:]]}
    one = m.sample_log(cond1, steps=1, zT=fx["zT"][1:])
    check(one, fx["sample"][1:], "sample_log, one row", l2=0.015, worst=0.02)
    # and a drawn zT has the right shape / statistics
    drawn = m.sample_log(cond1, steps=1)
    assert drawn.shape == (1, 4, 16, 16) and torch.isfinite(drawn).all()


def test_apply_condition_encoder_vs_reference_fixture(small):
    m, _ = small
    fx = load("cldm_small.npz")
    lat = m.apply_condition_encoder(fx["cond_control"])
    check(lat, fx["cond_latent"], "apply_condition_encoder vs reference", l2=0.02, worst=0.015)


def test_log_images_pipeline_vs_oracle(small):
    """The whole chain in one ir_cldm_pipeline call: SwinIR -> condition encoder -> ControlNet + UNet -> decoder, against the oracle."""
    m, sds = small
    B, H, W = 2, 128, 192
    lq = det_input(81, (B, H, W, 3))
    zT = det_input(82, (B, 4, H // 8, W // 8), -2.0, 2.0)
    ctxt = det_input(71, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0)
    got = m.log_images({"hint": lq}, zT=zT, c_crossattn=ctxt[0])
    x = lq.permute(0, 3, 1, 2)
    control = oswin.swinir_forward(sds["swin"], x, SWIN_SMALL)
    c_latent = ovae.vae_encode_mean(sds["vae"], control * 2 - 1, dict(ch=32)) * 0.18215
    sd = {**{"model.diffusion_model." + k: v for k, v in sds["unet"].items()}, **{"control_model." + k: v for k, v in sds["cnet"].items()}}
    z = ocldm.reflow_sample(sd, zT, c_latent, ctxt.expand(B, -1, -1), CLDM_SMALL)
    ref = (ovae.vae_decode(sds["vae"], z / 0.18215, dict(ch=32)) + 1) / 2
    check(got["control"], control, "pipeline: control image (SwinIR)", l2=0.008, worst=0.015)
    check(got["samples"], ref, "pipeline: samples", l2=0.03, worst=0.03)
    # stage by stage through the host mirror gives the same result as the fused call
    cond = {"c_concat": [got["control"]], "c_crossattn": [ctxt.expand(B, -1, -1).contiguous()], "c_latent": [m.apply_condition_encoder(got["control"])]}
    staged = (m.decode_first_stage(m.sample_log(cond, zT=zT)) + 1) / 2
    check(staged, got["samples"], "staged vs fused", l2=1e-3, worst=2e-3)
    # recorded as a hipGraph (capture on the first call, replay on the second, on other inputs in between): the same bits
    g1 = m.log_images({"hint": lq}, zT=zT, c_crossattn=ctxt[0], graph=True)
    m.log_images({"hint": det_input(83, (B, H, W, 3))}, zT=det_input(84, (B, 4, H // 8, W // 8), -2.0, 2.0), c_crossattn=ctxt[0], graph=True)
    g2 = m.log_images({"hint": lq}, zT=zT, c_crossattn=ctxt[0], graph=True)
    for k in ("control", "samples"):
        assert torch.equal(g1[k], got[k]) and torch.equal(g2[k], got[k]), f"graph form differs in {k}"


def test_full_width_unet_vs_oracle():
    """configs/cldm.yaml widths (320 x [1, 2, 4, 4], 64-channel heads, 1024-wide context): GroupNorm over 320 ... 2560 channels, 1280-wide
    LayerNorm / GEGLU, head dim 64, at a 32 x 32 latent, ControlNet + UNet against the oracle."""
    from instarevive_amd.cldm import ControlledUnetModel, ControlNet, _sample
    cfg = dict(ocldm.DEFAULT_CFG)
    sd_u = det_state_dict(ocldm.state_dict_shapes(cfg), seed=717)
    sd_c = det_state_dict(ocldm.state_dict_shapes(cfg, control=True), seed=718)
    params = dict(image_size=32, in_channels=4, model_channels=320, attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4],
                  num_head_channels=64, use_spatial_transformer=True, use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, legacy=False)
    unet, cnet = ControlledUnetModel(out_channels=4, **params), ControlNet(hint_channels=4, **params)
    unet.load_state_dict(sd_u)
    cnet.load_state_dict(sd_c)
    unet.to("cuda"); cnet.to("cuda")
    zT, c_latent = det_input(91, (1, 4, 32, 32), -2.0, 2.0), det_input(92, (1, 4, 32, 32), -2.0, 2.0)
    ctxt = det_input(93, (1, 77, 1024), -1.0, 1.0)
    got = _sample(unet.ctx, zT, c_latent, 999.0, ctxt, add_x=True)
    sd = {**{"model.diffusion_model." + k: v for k, v in sd_u.items()}, **{"control_model." + k: v for k, v in sd_c.items()}}
    ref = ocldm.reflow_sample(sd, zT, c_latent, ctxt, cfg)
    check(got, ref, "full-width ControlNet + UNet vs oracle")


def test_each_control_residual_alone(small):
    """Each of the 13 control residuals (zero_conv_i(g_i) + hs_i written into its slice of a decoder input, middle_block_out into the first
    decoder block's h) one at a time: with a ControlNet whose zero-convs are all zero except number i, sample_log with control minus sample_log
    without control against the same difference through oracle/cldm.py - rel-L2 ON THE DIFFERENCE, so a residual that is lost, scaled or lands
    in another slice gives 1.0 or more where the whole-output gate sees 1.0 - 9.7 x its 1.8 % (residuals 11 and 12: 1.01 and 1.03 x). Gates:
    unet_block_ref.RESIDUAL_GATES = 2 x the bf16 emulation of that difference, derived on the CPU by tests/test_unet_block_ref_cpu.py
    (0.038 for residual 0 ... 0.32 for number 12: the rounding noise of two runs against an effect of 17 % ... 3.5 % of the output). No zero-conv
    needed scaling. Measured on the MI355X: see docs/parity.md, "ControlLDM blocks"."""
    from tests.support import unet_block_ref as R
    m, sds = small
    assert R.CLDM_SMALL == CLDM_SMALL and R.RESIDUAL_SEEDS["unet"] == 707 and R.RESIDUAL_SEEDS["cnet"] == 708   # the weights the gates were derived on
    zT, c_latent, ctxt = R.residual_inputs()
    t = torch.full((1,), 999.0)
    cond = lambda cl: {"c_concat": [torch.zeros(1, 3, 128, 128)], "c_crossattn": [ctxt], "c_latent": cl}
    bare_ref = zT + ocldm.unet_forward(sds["unet"], zT, t, ctxt, None, CLDM_SMALL)
    bare = m.sample_log(cond(None), zT=zT).float().cpu()
    failed = []
    try:
        for i in range(R.N_RESIDUALS):
            sd_i = R.only_residual(sds["cnet"], i)
            m.control_model.load_state_dict(sd_i)
            got = m.sample_log(cond([c_latent]), zT=zT).float().cpu() - bare
            ref = zT + ocldm.unet_forward(sds["unet"], zT, t, ctxt, ocldm.controlnet_forward(sd_i, zT, c_latent, t, ctxt, CLDM_SMALL), CLDM_SMALL) - bare_ref
            assert torch.isfinite(got).all(), i
            e = float((got - ref).norm() / ref.norm())
            print(f"control residual {i:2d} alone: rel-L2 on the difference {e:.4f} (gate {R.RESIDUAL_GATES[i]:.3f}; |difference| / |output| {float(ref.norm() / bare_ref.norm()):.3f})")
            if not e <= R.RESIDUAL_GATES[i]:
                failed.append((i, e, R.RESIDUAL_GATES[i]))
    finally:
        m.control_model.load_state_dict(sds["cnet"])
    assert not failed, f"(residual, rel-L2 on the difference, gate): {failed}"


def test_errors_are_loud(small):
    m, _ = small
    with pytest.raises(NotImplementedError):
        m.get_learned_conditioning([""])
    with pytest.raises(ValueError):   # two different prompts in one call
        bad = torch.randn(2, 77, CLDM_SMALL["context_dim"])
        m.sample_log({"c_concat": [torch.zeros(2, 3, 128, 128)], "c_crossattn": [bad], "c_latent": None}, zT=torch.zeros(2, 4, 16, 16))
    with pytest.raises(RuntimeError):  # latent not a multiple of 8 (three stride-2 levels)
        ctxt = torch.zeros(1, 77, CLDM_SMALL["context_dim"])
        m.sample_log({"c_concat": [torch.zeros(1, 3, 96, 96)], "c_crossattn": [ctxt], "c_latent": None}, zT=torch.zeros(1, 4, 12, 12))


def test_nonsquare_timestep_and_context_changes(small):
    """A non-square latent against the oracle; the per-timestep tables (emb_layers folded into the conv biases) and the per-context K / V caches
    are rebuilt when the timestep / context changes and give the first result again when it changes back."""
    m, sds = small
    B, h, w = 1, 16, 24
    zT, c_latent = det_input(61, (B, 4, h, w), -2.0, 2.0), det_input(62, (B, 4, h, w), -2.0, 2.0)
    ctx_a = det_input(63, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0)
    ctx_b = det_input(64, (1, 50, CLDM_SMALL["context_dim"]), -1.0, 1.0)   # another prompt length (50 tokens)
    sd = {**{"model.diffusion_model." + k: v for k, v in sds["unet"].items()}, **{"control_model." + k: v for k, v in sds["cnet"].items()}}
    cond = lambda c: {"c_concat": [torch.zeros(B, 3, 8 * h, 8 * w)], "c_crossattn": [c], "c_latent": [c_latent]}
    first = m.sample_log(cond(ctx_a), zT=zT)
    check(first, ocldm.reflow_sample(sd, zT, c_latent, ctx_a, CLDM_SMALL), "16 x 24 latent vs oracle")
    t = torch.full((B,), 500.0)
    eps500 = m.apply_model(zT, t, cond(ctx_a))
    ref500 = ocldm.unet_forward(sds["unet"], zT, t, ctx_a, ocldm.controlnet_forward(sds["cnet"], zT, c_latent, t, ctx_a, CLDM_SMALL), CLDM_SMALL)
    check(eps500, ref500, "apply_model at t = 500 vs oracle")
    other = m.sample_log(cond(ctx_b), zT=zT)
    check(other, ocldm.reflow_sample(sd, zT, c_latent, ctx_b, CLDM_SMALL), "50-token context vs oracle")
    assert float((other.cpu() - first.cpu()).abs().max()) > 1e-3
    again = m.sample_log(cond(ctx_a), zT=zT)
    assert torch.equal(again.cpu(), first.cpu())


def test_pipeline_hipgraph_replay_is_identical(small):
    from instarevive_amd import _lib as L
    from instarevive_amd.cldm import _set_context
    m, _ = small
    ctx = m.ctx
    n, h, w = 1, 128, 128
    lq = det_input(51, (n, 3, h, w)).cuda()
    zT = det_input(52, (n, 4, h // 8, w // 8), -2.0, 2.0).cuda()
    _set_context(ctx, det_input(71, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0))
    m._ready(); m.preprocess_model._ready()
    ws = ctx.workspace(ctx.ws_bytes(L.STAGE_CLDM_PIPELINE, n, h, w))
    outs = []
    for flags in (0, L.FLAG_GRAPH, L.FLAG_GRAPH, 0):   # plain, record + first replay, replay, plain
        out = torch.zeros_like(lq)
        if flags:
            out = outs[1] if len(outs) > 1 else out   # a graph is keyed by its pointers: replay into the same buffer
        ctx.check(ctx.lib.ir_cldm_pipeline(ctx.h, ctx.stream(), L.ptr(lq), L.ptr(zT), L.ptr(out), None, n, h, w, flags, 999.0, 0.18215, L.ptr(ws), ws.numel()),
                  "ir_cldm_pipeline")
        torch.cuda.synchronize()
        outs.append(out.clone() if flags else out)
    assert float(outs[0].std()) > 1e-3
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


CLIP_SMALL = dict(width=128, heads=4, layers=4, vocab_size=1000, context_length=77, mlp_ratio=4.0)


def test_clip_text_tower_vs_oracle():
    """FrozenOpenCLIPEmbedder (layer "penultimate": 3 of the 4 blocks run) against oracle/clip_text.py on deterministic weights: random token
    ids, the empty prompt through the built-in tokenisation, an id outside the vocabulary, and its use as get_unconditional_conditioning."""
    from instarevive_amd.cldm import FrozenOpenCLIPEmbedder
    from oracle import clip_text as oclip
    cfg = dict(CLIP_SMALL, layer="penultimate")
    sd = det_state_dict(oclip.state_dict_shapes(cfg), seed=909)
    enc = FrozenOpenCLIPEmbedder(layer="penultimate", width=128, heads=4, layers=4, vocab_size=1000)
    enc.load_state_dict({"model." + k: v for k, v in sd.items()})
    enc.to("cuda")
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, 1000, (3, 77), generator=g)
    check(enc.encode_with_transformer(tokens), oclip.encode_with_transformer(sd, tokens, cfg), "CLIP text tower (penultimate) vs oracle", l2=0.008, worst=0.015)
    last = FrozenOpenCLIPEmbedder(layer="last", width=128, heads=4, layers=4, vocab_size=1000)
    last.load_state_dict(sd)
    last.to("cuda")
    check(last.encode_with_transformer(tokens[:1]), oclip.encode_with_transformer(sd, tokens[:1], dict(cfg, layer="last")), "CLIP text tower (last) vs oracle",
          l2=0.008, worst=0.015)
    enc._ready()
    assert enc.tokenize(["", ""]).tolist() == [[49406, 49407] + [0] * 75] * 2   # open_clip.tokenize(""): <start_of_text>, <end_of_text>, zero padding
    with pytest.raises(RuntimeError):   # ... which is outside this 1000-entry test vocabulary: loud, like the reference's nn.Embedding
        enc([""])
    big = FrozenOpenCLIPEmbedder(layer="penultimate", width=128, heads=4, layers=2, vocab_size=49408)
    sd_big = det_state_dict(oclip.state_dict_shapes(dict(cfg, layers=2, vocab_size=49408)), seed=910)
    big.load_state_dict(sd_big)
    big.to("cuda")
    e = big([""] * 2)   # the reference's get_unconditional_conditioning
    check(e, oclip.encode_with_transformer(sd_big, big.tokenize(["", ""]), dict(cfg, layers=2, vocab_size=49408)), "empty prompt vs oracle", l2=0.008, worst=0.015)
    assert torch.equal(e[0], e[1])
    enc._ready()
    with pytest.raises(NotImplementedError):
        enc(["a photo"])
    with pytest.raises(RuntimeError):
        enc.encode_with_transformer(torch.full((1, 77), 1000))


def test_unconditional_conditioning_through_the_model():
    """get_unconditional_conditioning (cldm.py:529-530: the empty prompt through cond_stage_model) feeding sample_log, as the reference's samplers
    do - the text tower, the ControlNet and the UNet of one checkpoint on one device."""
    from oracle import clip_text as oclip
    ccfg = dict(width=CLDM_SMALL["context_dim"], heads=2, layers=3, vocab_size=49408, context_length=77, mlp_ratio=4.0, layer="penultimate")
    sd_clip = det_state_dict(oclip.state_dict_shapes(ccfg), seed=911)
    m, sds = make_cldm(clip=(dict(width=ccfg["width"], heads=2, layers=3, vocab_size=49408), sd_clip))
    c = m.get_unconditional_conditioning(2)
    ids = torch.zeros(2, 77, dtype=torch.long)
    ids[:, 0], ids[:, 1] = 49406, 49407
    c_ref = oclip.encode_with_transformer(sd_clip, ids, ccfg)
    check(c, c_ref, "get_unconditional_conditioning vs oracle", l2=0.008, worst=0.015)
    zT, c_latent = det_input(65, (2, 4, 16, 16), -2.0, 2.0), det_input(66, (2, 4, 16, 16), -2.0, 2.0)
    out = m.sample_log({"c_concat": [torch.zeros(2, 3, 128, 128)], "c_crossattn": [c], "c_latent": [c_latent]}, zT=zT)
    sd = {**{"model.diffusion_model." + k: v for k, v in sds["unet"].items()}, **{"control_model." + k: v for k, v in sds["cnet"].items()}}
    check(out, ocldm.reflow_sample(sd, zT, c_latent, c_ref, CLDM_SMALL), "sample_log with the model's own conditioning vs oracle")


def test_clip_text_tower_full_size():
    """The ViT-H-14 text tower at its real size (width 1024, 16 heads x 64, 24 blocks of which 23 run, 49408-token vocabulary): the empty
    prompt the reference samples with, against the oracle."""
    from instarevive_amd.cldm import FrozenOpenCLIPEmbedder
    from oracle import clip_text as oclip
    cfg = dict(oclip.DEFAULT_CFG)
    sd = det_state_dict(oclip.state_dict_shapes(cfg), seed=912)
    enc = FrozenOpenCLIPEmbedder(layer="penultimate")
    enc.load_state_dict(sd)
    enc.to("cuda")
    got = enc([""])
    check(got, oclip.encode_with_transformer(sd, enc.tokenize([""]), cfg), "ViT-H-14 text tower, empty prompt", l2=0.008, worst=0.015)
