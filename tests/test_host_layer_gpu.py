"""The shared host paths of api.cpp at small shapes: the hipGraph record / replay cache behind ir_pipeline and ir_cldm_pipeline (graph_run), the
cross-attention K / V cache builders behind ir_dit_set_prompt, ir_dit_set_prompts and ir_unet_set_context. Every comparison here is bit for bit:
these paths choose buffers, strides and launch order, never arithmetic."""
import ctypes as C

import pytest
import torch

from instarevive_amd import _lib as L
from tests.golden._det import det_input
from tests.test_cldm_gpu import CLDM_SMALL, make_cldm
from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models, make_dit, make_dit_control
from tests.test_stage_args_gpu import _bind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cldm_small():
    return make_cldm()


def test_graph_cache_records_once_evicts_the_oldest_and_drops_on_a_new_generation(cldm_small):
    """ir_cldm_pipeline with IR_FLAG_GRAPH at 1 x 128 x 128 into fixed buffers: the recording call and the replay give the plain call's bits;
    one recording per key, the oldest of more than 16 keys is evicted, and a generation change (ir_set_fp8 on and off) drops every graph."""
    from instarevive_amd.cldm import _set_context
    m, _ = cldm_small
    ctx = m.ctx
    n, h, w = 1, 128, 128
    lq = det_input(51, (n, 3, h, w)).cuda()
    zT = det_input(52, (n, 4, h // 8, w // 8), -2.0, 2.0).cuda()
    _set_context(ctx, det_input(71, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0))
    m._ready(); m.preprocess_model._ready()
    ws = torch.empty(ctx.ws_bytes(L.STAGE_CLDM_PIPELINE, n, h, w), dtype=torch.uint8, device="cuda")
    plain_out, out = torch.zeros_like(lq), torch.zeros_like(lq)

    def call(t, flags=L.FLAG_GRAPH):
        """-> (the output, how many graphs the call recorded); a graph is keyed by its pointers, so every graph call writes `out`."""
        o, before = (out if flags else plain_out), ctx.graph_records
        ctx.check(ctx.lib.ir_cldm_pipeline(ctx.h, ctx.stream(), L.ptr(lq), L.ptr(zT), L.ptr(o), None, n, h, w, flags, float(t), 0.18215, L.ptr(ws), ws.numel()),
                  "ir_cldm_pipeline")
        torch.cuda.synchronize()
        return o.clone(), ctx.graph_records - before

    plain, recorded = call(999, 0)
    assert recorded == 0 and float(plain.std()) > 1e-3
    got, recorded = call(999)
    assert recorded == 1 and torch.equal(got, plain)
    got, recorded = call(999)
    assert recorded == 0 and torch.equal(got, plain)
    others = [100 + 50 * i for i in range(16)]
    assert [call(t)[1] for t in others] == [1] * 16
    got, recorded = call(999)   # the 16 entries are the 16 other timesteps: the first one was dropped
    assert recorded == 1 and torch.equal(got, plain)
    assert call(others[-1])[1] == 0
    assert ctx.lib.ir_set_fp8(ctx.h, 1) == 0 and ctx.lib.ir_set_fp8(ctx.h, 0) == 0
    assert call(others[-1])[1] == 1


def test_graph_replays_and_stage_calls_each_find_their_own_timestep_tables():
    """ir_pipeline with IR_FLAG_GRAPH (timestep 400, 1 x 64 x 128) around ir_dit_forward at timestep 700 on the same context: a recording and a
    replay both leave the DiT's cached timestep stale, so the stage call after either rebuilds its tables, and the replay rebuilds its own."""
    from instarevive_amd.models import DDPMScheduler
    from instarevive_amd.pipeline import _prepare_fused
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    ctx = dit.ctx
    n, h, w = 1, 64, 128
    _prepare_fused(dit, y.cuda(), mask3.cuda(), h, w, False, 0, others=(sw, vae))
    dit.ensure_pos(8, 8)
    img = (det_input(90, (n, h, w, 3)) * 255).to(torch.uint8).cuda()
    out, plain_out = torch.zeros_like(img), torch.zeros_like(img)
    lat = det_input(31, (1, 4, 16, 16), -2, 2).cuda()
    eps = torch.zeros(1, 8, 16, 16, device="cuda")
    ws = torch.empty(max(ctx.ws_bytes(L.STAGE_PIPELINE, n, h, w), ctx.ws_bytes(L.STAGE_DIT, 1, 16, 16)), dtype=torch.uint8, device="cuda")
    acp, sf = float(DDPMScheduler().alphas_cumprod[400]), float(vae.config.scaling_factor)

    def pipe(flags):
        o, before = (out if flags else plain_out), ctx.graph_records
        ctx.check(ctx.lib.ir_pipeline(ctx.h, ctx.stream(), L.ptr(img), L.ptr(o), None, n, h, w, flags, 0, 0, 400.0, acp, sf, L.ptr(ws), ws.numel()), "ir_pipeline")
        torch.cuda.synchronize()
        return o.clone(), ctx.graph_records - before

    def forward():
        ctx.check(ctx.lib.ir_dit_forward(ctx.h, ctx.stream(), L.ptr(lat), 700.0, L.ptr(eps), 1, 16, 16, L.ptr(ws), ws.numel()), "ir_dit_forward")
        torch.cuda.synchronize()
        return eps.clone()

    first = forward()
    rec, recorded = pipe(L.FLAG_GRAPH)
    assert recorded == 1 and float(rec.float().std()) > 1
    assert torch.equal(forward(), first)       # behind the recording call
    rep, recorded = pipe(L.FLAG_GRAPH)
    assert recorded == 0 and torch.equal(rep, rec)
    assert torch.equal(forward(), first)       # behind the replay
    assert torch.equal(pipe(0)[0], rec)


@pytest.mark.parametrize("control", [False, True])
def test_prompt_caches_of_both_setters_hold_the_same_bits(control):
    """ir_dit_set_prompt and ir_dit_set_prompts on the small DiT (with and without a control branch), prompts of 10 tokens (7 unmasked): a slot
    of set_prompts holds what set_prompt builds, and after every step of n_tok 10 -> 70 -> 10 (set_prompt: another 64-token bucket and back) and
    of P 2 -> 1 -> 3 (set_prompts: fewer slots reuse the caches, more re-allocate them) and back to set_prompt (slot 0 of the larger caches),
    ir_dit_forward gives the bits of a fresh context that was given the same prompts."""
    if control:
        model, _ = make_dit_control(dict(DIT_SMALL, num_layers=3), 2)
        parts = (model.base_model, model)
    else:
        model, _ = make_dit(DIT_SMALL)
        parts = (model,)
    lib, cap = L.load_library(), DIT_SMALL["caption_channels"]
    lat3 = det_input(31, (1, 4, 16, 16), -2, 2).cuda().expand(3, -1, -1, -1).contiguous()   # the same latent in every item
    cond3 = det_input(32, (1, 4, 16, 16), -2, 2).cuda().expand(3, -1, -1, -1).contiguous()
    y, z, v, y70 = (det_input(s, (t, cap), -1, 1) for s, t in ((9, 10), (10, 10), (11, 10), (12, 70)))
    bias10 = torch.zeros(10)
    bias10[7:] = -10000.0
    bias70 = torch.zeros(70)
    keep = []   # contexts, and the device operands of ir_dit_set_prompts, until the test ends

    def fresh():
        ctx = L.Context(0)
        _bind(ctx, *parts)
        parts[0].ensure_pos(8, 8)
        keep.append(ctx)
        return ctx

    def set_prompt(ctx, p, b):
        ctx.check(lib.ir_dit_set_prompt(ctx.h, ctx.stream(), C.c_void_p(p.data_ptr()), C.c_void_p(b.data_ptr()), p.shape[0]), "ir_dit_set_prompt")

    def set_prompts(ctx, ps):
        e, b = torch.stack(ps).cuda(), torch.stack([bias10] * len(ps)).cuda()
        keep.append((e, b))
        ctx.check(lib.ir_dit_set_prompts(ctx.h, ctx.stream(), L.ptr(e), L.ptr(b), len(ps), 10), "ir_dit_set_prompts")

    def forward(ctx, n):
        out = torch.zeros(n, 8, 16, 16, device="cuda")
        ws = ctx.workspace(ctx.ws_bytes(L.STAGE_DIT, n, 16, 16))
        if control:
            rc = lib.ir_dit_forward_control(ctx.h, ctx.stream(), L.ptr(lat3), L.ptr(cond3), 400.0, L.ptr(out), n, 16, 16, L.ptr(ws), ws.numel())
        else:
            rc = lib.ir_dit_forward(ctx.h, ctx.stream(), L.ptr(lat3), 400.0, L.ptr(out), n, 16, 16, L.ptr(ws), ws.numel())
        ctx.check(rc, "ir_dit_forward")
        torch.cuda.synchronize()
        return out

    # what a fresh context answers, once per prompt state
    ref = {}
    for name, ps in (("y", [y]), ("y70", [y70])):
        ctx = fresh()
        set_prompt(ctx, ps[0], bias70 if name == "y70" else bias10)
        ref[name] = forward(ctx, 1)
        if name == "y":
            ref["y for two"] = forward(ctx, 2)   # (another batch size may take other GEMM routes: two images are compared with two images)
    for name, ps in (("y,z", [y, z]), ("z", [z]), ("z,y,v", [z, y, v])):
        ctx = fresh()
        set_prompts(ctx, ps)
        ref[name] = forward(ctx, len(ps))
    assert float(ref["y"].std()) > 1e-3 and not torch.equal(ref["y"], ref["y70"]) and not torch.equal(ref["y"], ref["z"])

    ctx = fresh()
    set_prompt(ctx, y, bias10)
    assert torch.equal(forward(ctx, 1), ref["y"])
    set_prompts(ctx, [y])
    assert torch.equal(forward(ctx, 1), ref["y"]), "one slot of ir_dit_set_prompts differs from ir_dit_set_prompt"
    for p, ps in enumerate(([y, z], [z, y])):
        set_prompts(ctx, ps)
        assert torch.equal(forward(ctx, 2)[p], ref["y for two"][p]), f"item {p} of two prompts"
    for name, p, b in (("y", y, bias10), ("y70", y70, bias70), ("y", y, bias10)):
        set_prompt(ctx, p, b)
        assert torch.equal(forward(ctx, 1), ref[name]), f"ir_dit_set_prompt, n_tok {p.shape[0]}"
    for name, ps in (("y,z", [y, z]), ("z", [z]), ("z,y,v", [z, y, v])):
        set_prompts(ctx, ps)
        assert torch.equal(forward(ctx, len(ps)), ref[name]), f"ir_dit_set_prompts, P = {len(ps)}"
    set_prompt(ctx, y, bias10)
    assert torch.equal(forward(ctx, 1), ref["y"]), "ir_dit_set_prompt into slot 0 of caches sized for 3 prompts"


def test_unet_context_caches_are_rebuilt_for_another_length_and_back(cldm_small):
    """ir_unet_set_context with 77 tokens, then 50, then the 77 again on one context: ir_cldm_sample after the third gives the bits of the first."""
    from instarevive_amd.cldm import _sample
    m, _ = cldm_small
    m._ready()
    zT, c_latent = det_input(61, (1, 4, 16, 16), -2.0, 2.0), det_input(62, (1, 4, 16, 16), -2.0, 2.0)
    c77 = det_input(63, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0)
    c50 = det_input(64, (1, 50, CLDM_SMALL["context_dim"]), -1.0, 1.0)
    first = _sample(m.ctx, zT, c_latent, 999.0, c77, add_x=True).clone()
    other = _sample(m.ctx, zT, c_latent, 999.0, c50, add_x=True).clone()
    again = _sample(m.ctx, zT, c_latent, 999.0, c77, add_x=True)
    assert float(first.std()) > 1e-3 and not torch.equal(other, first)
    assert torch.equal(again, first)
