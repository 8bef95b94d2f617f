"""What the eight launching entry points of the image tools (api_image.cpp) refuse, and in which words: the return code and the whole ir_last_error
text of every bad argument against tests/golden/image_refusals.json. Host `if`s only: every call here is refused before anything is launched (all
buffers are real and larger than any call states, so a call that was wrongly let through would still stay inside them)."""
import ctypes as C
import json
import os

import pytest
import torch

from instarevive_amd import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_refusals.json")


def _off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


def _refusals():
    """{"<entry point>: <case>": [return code, ir_last_error]} on a fresh context (so that "not configured" is reachable)."""
    from instarevive_amd import clipiqa
    from tests.support import clipiqa_model as CM
    ctx = L.Context(0)
    lib, s = ctx.lib, ctx.stream()
    out = {}
    img = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    img2 = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    res = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")      # every tool's output: bytes, doubles or floats
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0 and res.data_ptr() % 8 == 0

    def run(tool, fn, defaults, cases):
        """fn(**arguments) -> return code; every case overrides some of `defaults`."""
        for name, over in cases.items():
            a = dict(defaults, **over)
            rc = int(fn(**a))
            assert rc != 0, f"{tool}: {name} was not refused"
            out[f"{tool}: {name}"] = [rc, lib.ir_last_error(a["c"]).decode()]

    def common(need, h, w, min_edge, align, img_keys=("img",), out_key="out", rows_key="rows", pitch_key="pitch"):
        """The cases every entry point with an image rectangle, a workspace and an output has."""
        cases = {"null context": dict(c=None), "null workspace": dict(ws=None), f"null {out_key}": {out_key: None}, "n = 0": dict(n=0),
                 "h below the minimum": dict(h=min_edge - 1), "w below the minimum": dict(w=min_edge - 1),
                 "workspace one byte short": dict(ws_bytes=need - 1)}
        for k in img_keys:
            cases[f"null {k}"] = {k: None}
        for k in (rows_key,) if isinstance(rows_key, str) else rows_key:
            cases[f"h = {k} + 1"] = {k: h - 1}
        for k in (pitch_key,) if isinstance(pitch_key, str) else pitch_key:
            cases[f"{k} = 3 w - 1"] = {k: 3 * w - 1}
        if align > 1:
            cases["workspace pointer off by one byte"] = dict(ws=_off(ws, 1))
        return cases

    # ---- PNG: 8 x 8 (no rows: the valid rectangle takes their place)
    need, bound = ctx.ws_bytes(L.STAGE_PNG, 1, 8, 8), int(lib.ir_png_bound(8, 8))
    info = torch.zeros(16, dtype=torch.int32, device="cuda")
    png = lambda c, img, n, h, w, pitch, vh, vw, out, out_stride, info, ws, ws_bytes: lib.ir_png_encode(c, s, img, n, h, w, pitch, vh, vw, out, out_stride, info, ws, ws_bytes)
    run("ir_png_encode", png, dict(c=ctx.h, img=L.ptr(img), n=1, h=8, w=8, pitch=24, vh=8, vw=8, out=L.ptr(res), out_stride=bound, info=L.ptr(info), ws=L.ptr(ws), ws_bytes=need),
        {"null context": dict(c=None), "null img": dict(img=None), "null out": dict(out=None), "null info": dict(info=None), "null workspace": dict(ws=None),
         "n = 0": dict(n=0), "h below the minimum": dict(h=0), "w below the minimum": dict(w=0), "vh = h + 1": dict(vh=9), "pitch = 3 w - 1": dict(pitch=23),
         "out_stride one byte short": dict(out_stride=bound - 1), "workspace one byte short": dict(ws_bytes=need - 1),
         "workspace pointer off by one byte": dict(ws=_off(ws, 1))})

    # ---- resampling: 8 x 8 -> 4 x 4, both passes (no rows: the full output size takes their place; the workspace is optional for one pass)
    need = ctx.ws_bytes(L.STAGE_RESAMPLE, 1, 8, 4)
    nplan = int(lib.ir_resample_plan_bytes(8, 8, 4, 4, L.RESAMPLE_BICUBIC))
    host_plan = torch.zeros(nplan + 4, dtype=torch.uint8)
    assert lib.ir_resample_plan(8, 8, 4, 4, L.RESAMPLE_BICUBIC, L.ptr(host_plan), nplan) == 0
    plan = host_plan.cuda()
    rsz = lambda c, img, n, in_h, in_w, in_pitch, out, out_h, out_w, full_h, full_w, out_pitch, plan, ws, ws_bytes: lib.ir_resample_u8(
        c, s, img, n, in_h, in_w, in_pitch, out, out_h, out_w, full_h, full_w, out_pitch, plan, ws, ws_bytes)
    run("ir_resample_u8", rsz, dict(c=ctx.h, img=L.ptr(img), n=1, in_h=8, in_w=8, in_pitch=24, out=L.ptr(res), out_h=4, out_w=4, full_h=4, full_w=4, out_pitch=12,
                                    plan=L.ptr(plan), ws=L.ptr(ws), ws_bytes=need),
        {"null context": dict(c=None), "null in": dict(img=None), "null out": dict(out=None), "null plan": dict(plan=None), "null workspace": dict(ws=None),
         "n = 0": dict(n=0), "in_h below the minimum": dict(in_h=0), "out_w below the minimum": dict(out_w=0), "out_h = full_h + 1": dict(full_h=3),
         "in_pitch = 3 in_w - 1": dict(in_pitch=23), "out_pitch = 3 full_w - 1": dict(out_pitch=11), "workspace one byte short": dict(ws_bytes=need - 1),
         "workspace pointer off by one byte": dict(ws=_off(ws, 1)), "plan pointer off by one byte": dict(plan=_off(plan, 1))})

    # ---- the paired metrics: PSNR-Y / SSIM-Y at 11 x 11, LPIPS at 31 x 31 (never configured here: every earlier check passes without weights)
    for tool, fn_, stage, e in (("ir_metrics_y", lib.ir_metrics_y, L.STAGE_METRICS, 11), ("ir_lpips", lib.ir_lpips, L.STAGE_LPIPS, 31)):
        need = ctx.ws_bytes(stage, 1, e, e)
        fn = lambda c, a, a_rows, a_pitch, b, b_rows, b_pitch, n, h, w, out, ws, ws_bytes, fn_=fn_: fn_(c, s, a, a_rows, a_pitch, b, b_rows, b_pitch, n, h, w, out, ws, ws_bytes)
        cases = common(need, e, e, e, 8, img_keys=("a", "b"), rows_key=("a_rows", "b_rows"), pitch_key=("a_pitch", "b_pitch"))
        cases["out off by four bytes"] = dict(out=_off(res, 4))
        if tool == "ir_lpips":
            cases["not configured"] = {}
        run(tool, fn, dict(c=ctx.h, a=L.ptr(img), a_rows=e, a_pitch=3 * e, b=L.ptr(img2), b_rows=e, b_pitch=3 * e, n=1, h=e, w=e, out=L.ptr(res), ws=L.ptr(ws), ws_bytes=need), cases)
    assert out["ir_lpips: not configured"][0] == L.LPIPS_NOT_CONFIGURED

    # ---- NIQE: 96 x 96
    need = ctx.ws_bytes(L.STAGE_NIQE, 1, 96, 96)
    fn = lambda c, img, rows, pitch, n, h, w, out, ws, ws_bytes: lib.ir_niqe_stats(c, s, img, rows, pitch, n, h, w, out, ws, ws_bytes)
    cases = common(need, 96, 96, 96, 8)
    cases["out off by four bytes"] = dict(out=_off(res, 4))
    run("ir_niqe_stats", fn, dict(c=ctx.h, img=L.ptr(img), rows=96, pitch=288, n=1, h=96, w=96, out=L.ptr(res), ws=L.ptr(ws), ws_bytes=need), cases)

    # ---- ir_degrade: 16 x 16 with a 3 x 3 blur; ir_degrade_chain: 16 x 16 with one filter op
    blur = torch.full((9,), 1.0 / 9.0, dtype=torch.float64, device="cuda")
    params = (L.DegradeParams * 1)()
    params[0].kernel, params[0].noise, params[0].ksize, params[0].lh, params[0].lw, params[0].q, params[0].norm, params[0].sigma = blur.data_ptr(), None, 3, 8, 8, 50, 0, 0.0
    chains = (L.Chain * 1)()
    chains[0].n_ops, chains[0].tap = 1, -1
    chains[0].ops[0].kind, chains[0].ops[0].a, chains[0].ops[0].data = 1, 3, blur.data_ptr()    # IR_CHAIN_FILTER, K = 3
    for tool, fn_, key, recs, need in (("ir_degrade", lib.ir_degrade, "params", params, ctx.ws_bytes(L.STAGE_DEGRADE, 1, 16, 16)),
                                       ("ir_degrade_chain", lib.ir_degrade_chain, "chains", chains, ctx.ws_bytes(L.STAGE_DEGRADE_CHAIN, 1, 16, 16, 16, 16))):
        fn = lambda c, img, rows, pitch, n, h, w, recs, out, ws, ws_bytes, fn_=fn_: fn_(c, s, img, rows, pitch, n, h, w, recs, out, None, ws, ws_bytes)
        cases = common(need, 16, 16, 1, 256)
        cases[f"null {key}"] = dict(recs=None)
        run(tool, fn, dict(c=ctx.h, img=L.ptr(img), rows=16, pitch=48, n=1, h=16, w=16, recs=recs, out=L.ptr(res), ws=L.ptr(ws), ws_bytes=need), cases)

    # ---- CLIP-IQA: 32 x 32. Its workspace and alignment checks sit behind the configured check: the rectangle first, then the seeded small model is bound
    fn = lambda c, img, rows, pitch, n, h, w, out, ws, ws_bytes: lib.ir_clipiqa(c, s, img, rows, pitch, n, h, w, out, None, ws, ws_bytes)
    base = dict(c=ctx.h, img=L.ptr(img), rows=32, pitch=96, n=1, h=32, w=32, out=L.ptr(res), ws=L.ptr(ws), ws_bytes=ws.numel())
    cases = common(0, 32, 32, 32, 1, out_key="out")
    del cases["workspace one byte short"]
    cases["not configured"] = {}
    run("ir_clipiqa", fn, base, cases)
    assert out["ir_clipiqa: not configured"][0] == L.CLIPIQA_NOT_CONFIGURED
    clipiqa.configure(ctx, CM.model("small"))
    need = ctx.ws_bytes(L.STAGE_CLIPIQA, 1, 32, 32)
    assert 0 < need <= ws.numel()
    run("ir_clipiqa", fn, dict(base, ws_bytes=need), {"workspace one byte short": dict(ws_bytes=need - 1), "workspace pointer off by one byte": dict(ws=_off(ws, 1)),
                                                     "scores off by four bytes": dict(out=_off(res, 4))})
    torch.cuda.synchronize()
    assert not bool(res.any()), "a refused call wrote its output"
    return out


def test_every_bad_argument_is_refused_in_the_recorded_words():
    """Every case of _refusals() gives the recorded return code and the recorded ir_last_error, byte for byte (the messages hold sizes, no addresses).
    tests/golden/image_refusals.json was recorded on the GPU from the library of the commit before the image tools got their own translation unit and
    their shared argument checks, built in a checkout of its own and named by INSTAREVIVE_HIP_LIB:
        import json; from tests.test_image_args_gpu import _refusals, GOLDEN
        json.dump(_refusals(), open(GOLDEN, "w"), indent=1, sort_keys=True)
    so the file, not the code under test, says what each entry point answers."""
    want = json.load(open(GOLDEN))
    got = _refusals()
    for name in sorted(set(want) | set(got)):
        print(name, got.get(name))
    assert set(got) == set(want), set(got) ^ set(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert len(want) > 100 and all(rc < 0 for rc, _ in want.values())
