"""What the stage entry points of api.cpp refuse, and in which words: the four DiT forms, ir_pipeline, ir_cldm_pipeline, the three K / V cache
setters and the two text encoders - the return code and the whole ir_last_error text of every bad call against tests/golden/stage_refusals.json.
Host `if`s only: every call here is refused before anything is launched (all buffers are real and larger than any call states, so a call that
was wrongly let through would still stay inside them); the one exception is the token id outside the vocabulary, which the small encoder finds."""
import ctypes as C
import json
import os

import pytest
import torch

from instarevive_amd import _lib as L
from tests.golden._det import det_input

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_refusals.json")


def _bind(ctx, *models):
    """Upload and configure models on `ctx` instead of the per-GPU context their .to() chose (so that "not configured" stays reachable here)."""
    for m in models:
        m.ctx, m.device = ctx, ctx.device
        m._upload()


def _refusals():
    """{"<entry point>: <case>": [return code, ir_last_error]}, each model family on a fresh context that is configured step by step."""
    from instarevive_amd.cldm import FrozenOpenCLIPEmbedder, _set_context
    from instarevive_amd.models import ControlTransformerHalf
    from oracle import clip_text as oclip
    from tests.golden._det import det_state_dict
    from tests.support.small_models import small_models
    from tests.test_cldm_gpu import CLDM_SMALL, CLIP_SMALL, make_cldm
    from tests.test_models_gpu import make_t5
    from tests.test_oracle_golden import T5_SMALL
    lib = L.load_library()
    out = {}
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")
    lat, cond, res = f32(1 << 20), f32(1 << 20), f32(1 << 22)      # every call's latents / images, and every call's output
    emb, bias = f32(30000 * 10 * 64), f32(30000 * 10)              # ir_dit_set_prompts' operands at the largest count tried
    host = torch.zeros(1 << 20, dtype=torch.float32)               # the host operands of ir_dit_set_prompt / ir_unet_set_context
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    hp = lambda t: C.c_void_p(t.data_ptr())

    def run(ctx, tool, fn, defaults, cases):
        """fn(**arguments) -> return code; every case overrides some of `defaults`."""
        for name, over in cases.items():
            a = dict(defaults, **over)
            rc = int(fn(**a))
            assert rc != 0, f"{tool}: {name} was not refused"
            assert f"{tool}: {name}" not in out
            out[f"{tool}: {name}"] = [rc, lib.ir_last_error(a["c"]).decode()]

    # ---- the DiT family: the four entry forms, ir_pipeline and the two prompt setters, one context configured step by step
    d = L.Context(0)
    s = d.stream()
    dit4 = dict(c=d.h, lat=L.ptr(lat), cond=L.ptr(cond), out=L.ptr(res), n=1, h=16, w=16, t=400.0, acp=0.5, ws=L.ptr(ws), ws_bytes=ws.numel())
    entries = {
        "ir_dit_forward": lambda c, lat, cond, out, n, h, w, t, acp, ws, ws_bytes: lib.ir_dit_forward(c, s, lat, t, out, n, h, w, ws, ws_bytes),
        "ir_dit_step": lambda c, lat, cond, out, n, h, w, t, acp, ws, ws_bytes: lib.ir_dit_step(c, s, lat, out, n, h, w, t, acp, ws, ws_bytes),
        "ir_dit_forward_control": lambda c, lat, cond, out, n, h, w, t, acp, ws, ws_bytes: lib.ir_dit_forward_control(c, s, lat, cond, t, out, n, h, w, ws, ws_bytes),
        "ir_dit_step_control": lambda c, lat, cond, out, n, h, w, t, acp, ws, ws_bytes: lib.ir_dit_step_control(c, s, lat, cond, out, n, h, w, t, acp, ws, ws_bytes)}
    base, control = ("ir_dit_forward", "ir_dit_step"), ("ir_dit_forward_control", "ir_dit_step_control")

    def dit_cases(names, cases):
        for tool in names:
            run(d, tool, entries[tool], dit4, {k: v for k, v in cases.items() if "acp" not in k or "step" in tool})

    pipe = lambda c, img, out, stage1, n, h, w, flags, t, acp, sf, ws, ws_bytes: lib.ir_pipeline(c, s, img, out, stage1, n, h, w, flags, 64, 32, t, acp, sf, ws, ws_bytes)
    pipe_d = dict(c=d.h, img=L.ptr(lat), out=L.ptr(res), stage1=None, n=1, h=64, w=64, flags=0, t=400.0, acp=0.5, sf=0.18215, ws=L.ptr(ws), ws_bytes=ws.numel())
    set1 = lambda c, e, b, n_tok: lib.ir_dit_set_prompt(c, s, e, b, n_tok)
    set1_d = dict(c=d.h, e=hp(host), b=hp(host), n_tok=10)
    setp = lambda c, e, b, p, n_tok: lib.ir_dit_set_prompts(c, s, e, b, p, n_tok)
    setp_d = dict(c=d.h, e=L.ptr(emb), b=L.ptr(bias), p=2, n_tok=10)

    dit_cases(base + control, {"null context": dict(c=None), "not configured": {}})
    run(d, "ir_pipeline", pipe, pipe_d, {"null context": dict(c=None), "not configured": {}})
    run(d, "ir_dit_set_prompt", set1, set1_d, {"null context": dict(c=None), "not configured": {}})
    run(d, "ir_dit_set_prompts", setp, setp_d, {"null context": dict(c=None), "not configured": {}})
    swin, vae, dit, _ = small_models()
    _bind(d, vae, dit)
    dit.ensure_pos(8, 8)
    dit_cases(base + control, {"prompt not set": {}})
    run(d, "ir_pipeline", pipe, pipe_d, {"prompt not set": dict(flags=L.FLAG_NO_PREPROCESS)})
    run(d, "ir_dit_set_prompt", set1, set1_d, {"null embeds": dict(e=None), "null bias": dict(b=None), "n_tok = 0": dict(n_tok=0)})
    run(d, "ir_dit_set_prompts", setp, setp_d, {"null embeds": dict(e=None), "null bias": dict(b=None), "n_tok = 0": dict(n_tok=0), "n_prompts = 0": dict(p=0),
                                                "30000 prompts overflow 2^31 elements": dict(p=30000)})
    cap = dit.cfg["caption_channels"]
    y3 = det_input(9, (3, 10, cap), -1, 1)

    def prompts(p):   # p different prompts of 10 tokens, through the setter of that count
        dit._set_prompt_rows(y3[:p].contiguous(), torch.zeros(p, 10), stream_ordered=False)

    prompts(2)
    dit_cases(base, {"2 prompts for a batch of 3": dict(n=3)})
    run(d, "ir_pipeline", pipe, pipe_d, {"SwinIR not configured": {}, "acp = 0": dict(flags=L.FLAG_NO_PREPROCESS, acp=0.0), "acp = 1": dict(flags=L.FLAG_NO_PREPROCESS, acp=1.0),
                                         "sf = 0": dict(flags=L.FLAG_NO_PREPROCESS, sf=0.0), "IR_FLAG_CONTROL_LQ without a control branch": dict(flags=L.FLAG_NO_PREPROCESS | L.FLAG_CONTROL_LQ),
                                         "2 prompts for a batch of 3": dict(flags=L.FLAG_NO_PREPROCESS, n=3)})
    prompts(1)
    _bind(d, swin)
    sizes = {"odd h": dict(h=15), "acp = 0": dict(acp=0.0), "acp = 1": dict(acp=1.0), "no dit.pos table for a 12 x 12 latent": dict(h=12, w=12)}
    dit_cases(base, sizes)
    dit_cases(control, {"no control branch": {}})
    run(d, "ir_pipeline", pipe, pipe_d, {"h = 65": dict(h=65), "n = 0": dict(n=0), "IR_FLAG_GRAPH with ws_bytes = 0": dict(flags=L.FLAG_GRAPH, ws_bytes=0)})
    assert d.graph_records == 0
    dit.ctx = None   # (the wrapper would otherwise move its base model to the per-GPU context)
    ctl = ControlTransformerHalf(dit, copy_blocks_num=1)
    _bind(d, dit, ctl)
    dit.ensure_pos(8, 8)
    dit_cases(control, {"control branch configured, prompt not set": {}})
    prompts(2)
    dit_cases(control, {"2 prompts for a batch of 3": dict(n=3)})
    prompts(1)
    dit_cases(control, dict(sizes, **{"null cond": dict(cond=None)}))

    # ---- the ControlLDM family: ir_cldm_pipeline and ir_unet_set_context
    u = L.Context(0)
    s = u.stream()
    cl = lambda c, lq, zT, out, n, h, w, flags, t, sf, ws, ws_bytes: lib.ir_cldm_pipeline(c, s, lq, zT, out, None, n, h, w, flags, t, sf, ws, ws_bytes)
    cl_d = dict(c=u.h, lq=L.ptr(lat), zT=L.ptr(cond), out=L.ptr(res), n=1, h=128, w=128, flags=0, t=999.0, sf=0.18215, ws=L.ptr(ws), ws_bytes=ws.numel())
    setc = lambda c, e, n_tok: lib.ir_unet_set_context(c, s, e, n_tok)
    setc_d = dict(c=u.h, e=hp(host), n_tok=77)
    run(u, "ir_cldm_pipeline", cl, cl_d, {"null context": dict(c=None), "not configured": {}})
    run(u, "ir_unet_set_context", setc, setc_d, {"null context": dict(c=None), "not configured": {}})
    m, _ = make_cldm()
    _bind(u, m.model.diffusion_model, m.control_model)
    run(u, "ir_unet_set_context", setc, setc_d, {"null context_host": dict(e=None), "n_tok = 0": dict(n_tok=0)})
    run(u, "ir_cldm_pipeline", cl, cl_d, {"no context set": {}})
    _set_context(u, det_input(71, (1, 77, CLDM_SMALL["context_dim"]), -1.0, 1.0))
    run(u, "ir_cldm_pipeline", cl, cl_d, {"VAE not configured": {}})
    _bind(u, m.first_stage_model)
    run(u, "ir_cldm_pipeline", cl, cl_d, {"SwinIR not configured": {}})
    _bind(u, m.preprocess_model)
    run(u, "ir_cldm_pipeline", cl, cl_d, {"null lq": dict(lq=None), "null zT": dict(zT=None), "null samples": dict(out=None), "scale_factor = 0": dict(sf=0.0),
                                          "h = 65": dict(h=65), "n = 0": dict(n=0), "IR_FLAG_GRAPH with ws_bytes = 0": dict(flags=L.FLAG_GRAPH, ws_bytes=0)})
    assert u.graph_records == 0
    torch.cuda.synchronize()
    assert not bool(res.any()), "a refused call wrote its output"

    # ---- the text encoders (their outputs go to a buffer of their own: the last case of each runs the small encoder)
    e = L.Context(0)
    s = e.stream()
    ids = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    txt = f32(1 << 22)
    t5f = lambda c, ids, out, b, t, ws, ws_bytes: lib.ir_t5_encode(c, s, ids, None, out, b, t, ws, ws_bytes)
    t5_d = dict(c=e.h, ids=L.ptr(ids), out=L.ptr(txt), b=1, t=8, ws=L.ptr(ws), ws_bytes=ws.numel())
    clf = lambda c, ids, out, b, ws, ws_bytes: lib.ir_clip_text_encode(c, s, ids, out, b, ws, ws_bytes)
    cl_d = dict(c=e.h, ids=L.ptr(ids), out=L.ptr(txt), b=1, ws=L.ptr(ws), ws_bytes=ws.numel())
    run(e, "ir_t5_encode", t5f, t5_d, {"null context": dict(c=None), "not configured": {}})
    run(e, "ir_clip_text_encode", clf, cl_d, {"null context": dict(c=None), "not configured": {}})
    t5, _ = make_t5(T5_SMALL)
    clip = FrozenOpenCLIPEmbedder(layer="penultimate", width=128, heads=4, layers=4, vocab_size=1000)
    clip.load_state_dict({"model." + k: v for k, v in det_state_dict(oclip.state_dict_shapes(dict(CLIP_SMALL, layer="penultimate")), seed=909).items()})
    _bind(e, t5, clip)
    t5(input_ids=torch.ones(1, 8, dtype=torch.long))   # uploads the position-bias table of 8 tokens
    run(e, "ir_t5_encode", t5f, t5_d, {"null ids": dict(ids=None), "null out": dict(out=None), "b = 0": dict(b=0), "t = 0": dict(t=0), "t = 513": dict(t=513),
                                       "no t5.bias table for 9 tokens": dict(t=9)})
    run(e, "ir_clip_text_encode", clf, cl_d, {"null ids": dict(ids=None), "null out": dict(out=None), "b = 0": dict(b=0)})
    torch.cuda.synchronize()
    assert not bool(txt.any()), "a refused call wrote its output"
    ids[5] = T5_SMALL["vocab_size"]
    run(e, "ir_t5_encode", t5f, t5_d, {"a token id equal to vocab": {}})
    ids[5] = CLIP_SMALL["vocab_size"]
    run(e, "ir_clip_text_encode", clf, cl_d, {"a token id equal to vocab": {}})
    ids[5] = 0   # the flag of the bad id is cleared with the refusal: the next good call passes
    assert t5f(**t5_d) == 0 and clf(**cl_d) == 0
    return out


def test_every_bad_call_is_refused_in_the_recorded_words():
    """Every case of _refusals() gives the recorded return code and the recorded ir_last_error, byte for byte (the messages hold sizes, no addresses).
    tests/golden/stage_refusals.json was recorded on the GPU from the library of the commit before these entry points got their shared graph
    cache, K / V cache filler and entry checks, built in a checkout of its own and named by INSTAREVIVE_HIP_LIB:
        import json; from tests.test_stage_args_gpu import _refusals, GOLDEN
        json.dump(_refusals(), open(GOLDEN, "w"), indent=1, sort_keys=True)
    so the file, not the code under test, says what each entry point answers."""
    want = json.load(open(GOLDEN))
    got = _refusals()
    for name in sorted(set(want) | set(got)):
        print(name, got.get(name))
    assert set(got) == set(want), set(got) ^ set(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert len(want) > 80 and all(rc < 0 for rc, _ in want.values())
