"""ir_lpips (csrc/lpips.hip) through the C ABI, the pipeline and the command line against the float64 model of tests/support/lpips_model.py.

The gate is measured from the reference, not from the kernel: the relative deviation of the fp32 host model (tools/evaluate_pairs.py::LPIPS on the
CPU) from the float64 model, the largest over all cases, times 8 (lpips_model.gate()). tests/test_lpips_cpu.py shows that every known way to
get AlexNet / LPIPS wrong lands at least 1.5 x outside it. The pooled figure and the device's worst deviation are printed by
test_every_case_passes_the_gate and recorded in docs/parity.md."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import lpips_model as LM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
_bound = {}


def _ctx(kind="normal"):
    """The shared context with the `kind` weights bound (re-bound only when the kind changes)."""
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if _bound.get("kind") != kind:
        for k, v in LM.weights(kind).items():
            ctx.upload(k, v)
        ctx.check(ctx.lib.ir_lpips_configure(ctx.h), "ir_lpips_configure")
        _bound["kind"] = kind
    return ctx


def _call(a_buf, b_buf, h, w, kind="normal"):
    """ir_lpips on a_buf [n][a_rows][a_pitch] / b_buf [n][b_rows][b_pitch] (bytes) -> [n] distances. The call gets exactly the workspace size the
    library reports; 4096 canary bytes behind it and four canary values behind out[n] must stay untouched."""
    ctx = _ctx(kind)
    n, a_rows, a_pitch = a_buf.shape
    _, b_rows, b_pitch = b_buf.shape
    da, db = torch.from_numpy(np.ascontiguousarray(a_buf)).cuda(), torch.from_numpy(np.ascontiguousarray(b_buf)).cuda()
    out = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_LPIPS, n, h, w)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    ctx.check(ctx.lib.ir_lpips(ctx.h, ctx.stream(), L.ptr(da), a_rows, a_pitch, L.ptr(db), b_rows, b_pitch, n, h, w, L.ptr(out), L.ptr(ws), need), "ir_lpips")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[n:] == OUT_CANARY), "values behind out[n] were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return res[:n].copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _embed(imgs, rows, pitch, seed):
    """The images in the top-left corner of [n][rows][pitch] buffers whose other bytes are noise."""
    buf = np.random.default_rng(seed).integers(0, 256, (len(imgs), rows, pitch), dtype=np.uint8)
    for i, im in enumerate(imgs):
        buf[i, :im.shape[0], :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    return buf


def _device_value(name):
    _, h, w, _, kind = next(c for c in LM.CASES if c[0] == name)
    a, b = LM.pair(name)
    return float(_call(_tight([a]), _tight([b]), h, w, kind)[0])


def test_every_case_passes_the_gate():
    """All cases in one test: the gate is pooled over them, and the dead-stage case needs its own binding once."""
    gate = LM.gate()
    print(f"pooled fp32 host deviation {LM.pooled_host_deviation():.3e}, gate {gate:.3e}")
    worst = 0.0
    devs = {}
    for name in [c[0] for c in LM.CASES if c[4] == "normal"] + [c[0] for c in LM.CASES if c[4] != "normal"]:
        got, ref = _device_value(name), LM.reference(name)
        devs[name] = LM.rel(got, ref)
        worst = max(worst, devs[name])
        print(f"{name}: device {got:.17g}, float64 model {ref:.17g}, off by {devs[name]:.3e} (host fp32: {LM.host_deviation(name):.3e})")
    print(f"device worst {worst:.3e}")
    assert all(np.isfinite(v) for v in devs.values())
    assert worst <= gate, (devs, gate)


def test_dead_stage_is_finite_and_within_the_gate():
    got, ref = _device_value("64x64_dead5"), LM.reference("64x64_dead5")
    assert np.isfinite(got) and LM.rel(got, ref) <= LM.gate(), (got, ref)
    # stage 5 is zero in both images: the same pair with the live weights must differ (the case is not vacuous)
    a, b = LM.pair("64x64_dead5")
    assert float(_call(_tight([a]), _tight([b]), 64, 64)[0]) != got


def test_identical_images_give_exactly_zero():
    a = LM.pair("97x130_ramps")[0]
    n = LM.pair("35x67_noise")[0]
    assert float(_call(_tight([a]), _tight([a.copy()]), 97, 130)[0]) == 0.0
    assert float(_call(_tight([n]), _tight([n.copy()]), 35, 67)[0]) == 0.0


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def test_batch_position_and_repetition_do_not_change_a_bit():
    """Three different pairs of 97 x 130 inside buffers of 111 / 103 rows and pitches of 401 / 397 bytes: per pair the bits of its single call."""
    h, w = 97, 130
    r = LM.pair("97x130_ramps")
    ps = [r, (LM.noise(h, w, 7), LM.noise(h, w, 8)), (r[1], LM.shifted(r[1], 3, 9))]
    a = _embed([p[0] for p in ps], 111, 401, 1)
    b = _embed([p[1] for p in ps], 103, 397, 2)
    batch = _call(a, b, h, w)
    singles = np.concatenate([_call(_tight([pa]), _tight([pb]), h, w) for pa, pb in ps])
    assert np.array_equal(_bits(batch), _bits(singles)), (batch, singles)
    assert LM.rel(batch[0], LM.reference("97x130_ramps")) <= LM.gate()
    again = _call(a, b, h, w)
    assert np.array_equal(_bits(again), _bits(batch))
    swapped = _call(a[[2, 0, 1]], b[[2, 0, 1]], h, w)
    assert np.array_equal(_bits(swapped), _bits(batch[[2, 0, 1]]))


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    h, w = 40, 33
    a = torch.from_numpy(LM.noise(h, w, 1)).cuda()
    b = torch.from_numpy(LM.noise(h, w, 2)).cuda()
    out = torch.full((6,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_LPIPS, 1, h, w)
    ws = torch.full((need + 4096,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pa=L.ptr(a), pb=L.ptr(b), po=L.ptr(out), pw=L.ptr(ws), wsb=need, b_rows=None, b_pitch=None):
        return ctx.lib.ir_lpips(ctx.h, ctx.stream(), pa, rows, pitch, pb, rows if b_rows is None else b_rows, pitch if b_pitch is None else b_pitch,
                                n, hh, ww, po, pw, wsb)

    assert call(n=0) == -1 and call(hh=30) == -1 and call(ww=30) == -1
    assert call(rows=h - 1) == -1 and call(b_rows=h - 1) == -1           # h above a_rows / b_rows
    assert call(pitch=3 * w - 1) == -1 and call(b_pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 8)) == -1                   # a misaligned one
    assert call(pa=None) == -1 and call(pb=None) == -1 and call(po=None) == -1 and call(pw=None) == -1
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[0]) > 0 and bool((out[1:] == OUT_CANARY).all()) and bool((ws[need:] == CANARY).all())


def test_a_context_without_lpips_weights_returns_its_own_code():
    ctx = L.Context(0)
    a = torch.from_numpy(LM.noise(31, 31, 1)).cuda()
    out = torch.full((2,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_LPIPS, 1, 31, 31)
    ws = torch.full((need,), CANARY, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.ir_lpips(ctx.h, ctx.stream(), L.ptr(a), 31, 93, L.ptr(a), 31, 93, 1, 31, 31, L.ptr(out), L.ptr(ws), need)
    assert rc == L.LPIPS_NOT_CONFIGURED and rc not in (0, -1)
    assert b"not configured" in ctx.lib.ir_last_error(ctx.h)
    # a missing tensor and one of another shape are named
    assert ctx.lib.ir_lpips_configure(ctx.h) < 0 and b"lpips.c1.w" in ctx.lib.ir_last_error(ctx.h)
    for k, v in LM.weights().items():
        ctx.upload(k, v[:-1] if k == "lpips.lin3" else v)
    assert ctx.lib.ir_lpips_configure(ctx.h) < 0 and b"lpips.lin3" in ctx.lib.ir_last_error(ctx.h)
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- host layer, pipeline
def _files(tmp_path, kind="normal", full=False):
    alex, lin = LM.state_dicts(LM.weights(kind), full=full)
    torch.save(lin, tmp_path / "lin.pth")
    if alex is not None:
        torch.save(alex, tmp_path / "alexnet.pth")
    return str(tmp_path / "lin.pth"), (str(tmp_path / "alexnet.pth") if alex is not None else None)


def test_lpips_arrays_from_weight_files(tmp_path):
    """lpips.configure from the two-file form and from one full state dict: the same bits, inside the gate."""
    from instarevive_amd import lpips as LP
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    _bound.clear()
    a, b = LM.pair("35x67_noise")
    lin, alex = _files(tmp_path)
    LP.configure(ctx, lin, alex)
    two = LP.lpips_arrays(ctx, a, b)
    os.makedirs(tmp_path / "full")
    lin, alex = _files(tmp_path / "full", full=True)
    assert alex is None
    LP.configure(ctx, lin)
    assert LP.lpips_arrays(ctx, a, b) == two and LM.rel(two, LM.reference("35x67_noise")) <= LM.gate()
    with pytest.raises(LP.LpipsError):
        LP.lpips_arrays(ctx, a[:30], b[:30])


def test_process_returns_triples_equal_to_a_standalone_call(tmp_path):
    """process(..., gt=, lpips=) on the reduced models: the third value of every score is ir_lpips of the returned image against its ground
    truth, the first two are what gt= alone gives, and without lpips= the return value is the pair form."""
    from instarevive_amd import lpips as LP
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support.metrics_model import ramp
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    _bound.clear()
    lin, alex = _files(tmp_path)
    LP.configure(dit.ctx, lin, alex)
    batch = [(det_input(500 + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    gts = [ramp(64, 128, 40), ramp(40, 100, 41)]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    preds, st1, (sp, s1) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=True, gt=gts, **kw)
    assert all(len(s) == 2 for s in sp + s1)
    preds3, st13, (sp3, s13) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=True, gt=gts, lpips=True, **kw)
    assert all(np.array_equal(x, z) for x, z in zip(preds + st1, preds3 + st13))
    assert all(len(s) == 3 for s in sp3 + s13)
    assert [s[:2] for s in sp3 + s13] == [tuple(s) for s in sp + s1]
    for arr, g, s in zip(preds3 + st13, gts + gts, sp3 + s13):
        alone = LP.lpips_arrays(dit.ctx, arr[:g.shape[0], :g.shape[1]], g)
        assert s[2] == alone and alone > 0, (s, alone)
    # the stream form, a batch without ground truth in between
    out = list(process_stream(dit, [batch, batch], "wavelet", False, False, 64, 32, gt=[None, gts], lpips=True, **kw))
    assert len(out[0]) == 2 and out[1][2][0] == sp3
    with pytest.raises(ValueError, match="lpips.*gt"):
        process(dit, batch, 1, "wavelet", False, False, 64, 32, lpips=True, **kw)
    with pytest.raises(ValueError, match="31 x 31"):
        process(dit, batch, 1, "wavelet", False, False, 64, 32, gt=[gts[0], ramp(30, 100, 1)], lpips=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_lpips_lin_adds_the_fourth_column(tmp_path):
    """inference.py --gt --lpips_lin --lpips_alexnet --png_encoder gpu --resize gpu over the 17-file folder of tests/test_metrics_gpu.py: metrics.csv
    has four columns whose last is ir_lpips of the decoded saved PNG against its ground truth, and the averages gain the `lpips:` line. The same
    command without --lpips_lin writes the three-column report."""
    from instarevive_amd import lpips as LP
    from instarevive_amd.metrics import read_report
    from instarevive_amd.models import get_context
    from tests.test_metrics_gpu import _cli_folder, _run
    d = tmp_path
    truth, cmd = _cli_folder(d)
    lin, alex = _files(d)
    cmd = cmd + ["--png_encoder", "gpu", "--resize", "gpu"]
    stdout = _run(cmd + ["--output", str(d / "out"), "--lpips_lin", lin, "--lpips_alexnet", alex])
    assert "were not scored" not in stdout and "--gt: scored 17 files" in stdout, stdout[-1500:]
    lines = (d / "out" / "metrics.csv").read_text().splitlines()
    assert lines[0] == "file,psnr_y,ssim_y,lpips" and len(lines) == 18 and all(len(ln.split(",")) == 4 for ln in lines)
    ctx = get_context(torch.device("cuda", 0))
    _bound.clear()
    LP.configure(ctx, lin, alex)
    got = read_report(str(d / "out" / "metrics.csv"))
    for k, g in truth.items():
        if min(g.shape[:2]) >= LP.MIN_EDGE:
            saved = np.array(Image.open(d / "out" / k).convert("RGB"))
            assert got[k][2] == LP.lpips_arrays(ctx, saved, g), k
    avg = [ln for ln in stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ", "lpips: "))]
    assert [ln.split(":")[0] for ln in avg] == ["psnr", "ssim", "lpips"]
    assert avg[2] == f"lpips: {np.mean([v[2] for v in got.values()]):.5f}"
    stdout = _run(cmd + ["--output", str(d / "plain")])
    assert (d / "plain" / "metrics.csv").read_text().splitlines()[0] == "file,psnr_y,ssim_y" and "lpips:" not in stdout
    assert read_report(str(d / "plain" / "metrics.csv")) == {k: v[:2] for k, v in got.items()}
