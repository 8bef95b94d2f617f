"""ir_dists (csrc/dists.hip) through the C ABI, the pipeline and the command line against the float64 model of tests/support/dists_model.py.

The gates are measured from the reference, not from the kernel: the absolute deviation of the fp32 host model (tools/evaluate_pairs.py::DISTS on
the CPU) from the float64 model, the largest over the cases, times 8 (dists_model.score_gate(); `40x24_flat` has its own), and per map and
moment kind the host model's max_c |m - ref| / max_c |ref|, pooled and multiplied alike (dists_model.moment_gate()). tests/test_dists_cpu.py
shows that every known way to get DISTS wrong lands outside the score gate. The figures are printed by the tests and recorded in
docs/parity.md."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import dists_model as DM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
MOM = DM.CHANNELS * 5
_bound = {}
_device = {}


def _ctx(kind="normal"):
    """The shared context with the `kind` weights bound (re-bound only when the kind changes)."""
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if _bound.get("kind") != kind:
        for k, v in DM.weights(kind).items():
            ctx.upload(k, v)
        ctx.check(ctx.lib.ir_dists_configure(ctx.h), "ir_dists_configure")
        _bound["kind"] = kind
    return ctx


def _call(a_buf, b_buf, h, w, kind="normal", moments=True, fill=CANARY):
    """ir_dists on a_buf [n][a_rows][a_pitch] / b_buf [n][b_rows][b_pitch] (bytes) -> ([n] scores, [n][1475][5] moments or None). The call gets
    exactly the workspace size the library reports, filled with `fill`; 4096 canary bytes behind it, four canary values behind out[n] and
    behind the moments must stay untouched."""
    ctx = _ctx(kind)
    n, a_rows, a_pitch = a_buf.shape
    _, b_rows, b_pitch = b_buf.shape
    da, db = torch.from_numpy(np.ascontiguousarray(a_buf)).cuda(), torch.from_numpy(np.ascontiguousarray(b_buf)).cuda()
    out = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    mom = torch.full((n * MOM + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_DISTS, n, h, w)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device="cuda")
    ws[need:] = CANARY
    assert ws.data_ptr() % 256 == 0
    ctx.check(ctx.lib.ir_dists(ctx.h, ctx.stream(), L.ptr(da), a_rows, a_pitch, L.ptr(db), b_rows, b_pitch, n, h, w, L.ptr(out), L.ptr(mom) if moments else None,
                               L.ptr(ws), need), "ir_dists")
    torch.cuda.synchronize()
    res, m = out.cpu().numpy(), mom.cpu().numpy()
    assert np.all(res[n:] == OUT_CANARY), "values behind out[n] were written"
    assert np.all(m[n * MOM if moments else 0:] == OUT_CANARY), "values behind the moments (or moments that were not asked for) were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return res[:n].copy(), (m[:n * MOM].reshape(n, DM.CHANNELS, 5).copy() if moments else None)


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
    """(score, moments [1475][5]) of a case on the device (computed once)."""
    if name not in _device:
        _, h, w, _, kind = DM.case(name)
        a, b = DM.pair(name)
        s, m = _call(_tight([a]), _tight([b]), h, w, kind)
        _device[name] = float(s[0]), m[0]
    return _device[name]


def _ordered():
    return [n for n in DM.NAMES if DM.case(n)[4] == "normal"] + [n for n in DM.NAMES if DM.case(n)[4] != "normal"]


def test_every_case_passes_the_gate():
    """All cases in one test: the gate is pooled over them, and the dead-stage case needs its own binding once."""
    print(f"pooled gate {DM.score_gate(DM.NAMES[0]):.3e}, gate of {DM.FLAT} {DM.score_gate(DM.FLAT):.3e}")
    devs = {}
    for name in _ordered():
        got, ref = _device_value(name)[0], DM.reference(name)[0]
        devs[name] = abs(got - ref)
        print(f"{name}: device {got:.17g}, float64 model {ref:.17g}, off by {devs[name]:.3e} (host fp32: {DM.host_deviation(name):.3e}, gate {DM.score_gate(name):.3e})")
    assert all(np.isfinite(v) for v in devs.values())
    assert all(devs[n] <= DM.score_gate(n) for n in DM.NAMES), devs


def test_moments_pass_their_gates():
    np.set_printoptions(precision=2, linewidth=200)
    print("pooled moment gate [map][mx, my, vx, vy, cxy]:\n", DM.moment_gate(DM.NAMES[0]))
    worst = np.zeros((len(DM.CHNS), 5))
    bad = {}
    for name in _ordered():
        got = DM.moment_measure(_device_value(name)[1], DM.reference(name)[1])
        if name != DM.FLAT:
            worst = np.maximum(worst, got)
        if not np.all(got <= DM.moment_gate(name)):
            bad[name] = got
    print("device worst (without the flat case):\n", worst)
    print(f"{DM.FLAT}: device\n", DM.moment_measure(_device_value(DM.FLAT)[1], DM.reference(DM.FLAT)[1]), "\ngate\n", DM.moment_gate(DM.FLAT))
    assert not bad, bad


def test_identical_images_score_zero():
    got, m = _device_value("33x18_same")
    assert abs(got) <= 1e-12, got
    assert np.array_equal(m[:, 0], m[:, 1]) and np.array_equal(m[:, 2], m[:, 3]) and np.array_equal(m[:, 2], m[:, 4])


def test_dead_stage_is_finite_and_within_the_gate():
    got, m = _device_value("64x64_dead5")
    assert np.isfinite(got) and np.all(np.isfinite(m)) and abs(got - DM.reference("64x64_dead5")[0]) <= DM.score_gate("64x64_dead5")
    assert np.all(m[DM.OFFSETS[5]:] == 0.0)   # stage 5 is zero in both images: S1 = S2 = 1 from the constants alone
    a, b = DM.pair("64x64_dead5")
    assert float(_call(_tight([a]), _tight([b]), 64, 64)[0][0]) != got   # with the live weights the pair scores differently: the case is not vacuous


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def test_batch_position_and_repetition_do_not_change_a_bit():
    """Three different pairs of 35 x 67 inside buffers of 41 / 37 rows and pitches of 211 / 203 bytes: per pair the bits of its single call,
    scores and moments, and the same scores without the moments."""
    h, w = 35, 67
    r = DM.pair("35x67_noise")
    ps = [r, (DM.ramp(h, w, 7), DM.ramp(h, w, 8)), (r[1], DM.shifted(r[1], 3, 9))]
    a = _embed([p[0] for p in ps], 41, 211, 1)
    b = _embed([p[1] for p in ps], 37, 203, 2)
    batch, bm = _call(a, b, h, w)
    singles = [_call(_tight([pa]), _tight([pb]), h, w) for pa, pb in ps]
    assert np.array_equal(_bits(batch), _bits(np.concatenate([s[0] for s in singles])))
    assert np.array_equal(_bits(bm), _bits(np.concatenate([s[1] for s in singles])))
    assert abs(batch[0] - DM.reference("35x67_noise")[0]) <= DM.score_gate("35x67_noise")
    again, am = _call(a, b, h, w)
    assert np.array_equal(_bits(again), _bits(batch)) and np.array_equal(_bits(am), _bits(bm))
    swapped, _ = _call(a[[2, 0, 1]], b[[2, 0, 1]], h, w)
    assert np.array_equal(_bits(swapped), _bits(batch[[2, 0, 1]]))
    plain, none = _call(a, b, h, w, moments=False)
    assert none is None and np.array_equal(_bits(plain), _bits(batch))


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    h, w = 40, 33
    a = torch.from_numpy(DM.noise(h, w, 1)).cuda()
    b = torch.from_numpy(DM.noise(h, w, 2)).cuda()
    out = torch.full((6,), OUT_CANARY, dtype=torch.float64, device="cuda")
    mom = torch.full((MOM + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_DISTS, 1, h, w)
    ws = torch.full((need + 4096,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pa=L.ptr(a), pb=L.ptr(b), po=L.ptr(out), pm=L.ptr(mom), pw=L.ptr(ws), wsb=need, b_rows=None, b_pitch=None):
        return ctx.lib.ir_dists(ctx.h, ctx.stream(), pa, rows, pitch, pb, rows if b_rows is None else b_rows, pitch if b_pitch is None else b_pitch,
                                n, hh, ww, po, pm, pw, wsb)

    assert call(n=0) == -1 and call(hh=15) == -1 and call(ww=15) == -1
    assert call(rows=h - 1) == -1 and call(b_rows=h - 1) == -1           # h above a_rows / b_rows
    assert call(pitch=3 * w - 1) == -1 and call(b_pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 8)) == -1                   # a misaligned one
    assert call(pa=None) == -1 and call(pb=None) == -1 and call(po=None) == -1 and call(pw=None) == -1
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((mom == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert 0 < float(out[0]) < 1 and bool((out[1:] == OUT_CANARY).all()) and bool((mom[MOM:] == OUT_CANARY).all()) and bool((ws[need:] == CANARY).all())
    assert bool((mom[:MOM] != OUT_CANARY).all())


def test_a_workspace_of_exactly_the_stated_bytes_of_ff_works():
    """The call reads nothing it has not written: a workspace of 0xFF bytes (NaN everywhere) gives the bits of the call above; the stated size
    is four stage-1 maps per pair plus the moment sums."""
    name = "35x67_noise"
    a, b = DM.pair(name)
    s, m = _call(_tight([a]), _tight([b]), 35, 67, fill=0xFF)
    assert np.array_equal(_bits(s), _bits(np.array([_device_value(name)[0]]))) and np.array_equal(_bits(m[0]), _bits(_device_value(name)[1]))
    ctx = _ctx()
    for n, h, w in ((1, 35, 67), (3, 16, 16), (2, 512, 512)):
        need, maps = ctx.ws_bytes(L.STAGE_DISTS, n, h, w), n * 4 * 64 * h * w * 4
        sizes, hh, ww = [(h, w), (h, w)], h, w
        for _ in range(4):
            hh, ww = (hh + 1) // 2, (ww + 1) // 2
            sizes.append((hh, ww))
        sums = max(c * ((a * b + 1023) // 1024) for c, (a, b) in zip(DM.CHNS, sizes))   # the 1024-pixel chunks x channels of the map where that is largest
        up = lambda x: (x + 255) // 256 * 256
        assert need == maps + up(n * sums * 40) + up(n * DM.CHANNELS * 40), (n, h, w, need, maps)
    assert ctx.ws_bytes(L.STAGE_DISTS, 1, 15, 64) == 0 and ctx.ws_bytes(L.STAGE_DISTS, 0, 64, 64) == 0


def test_a_context_without_dists_weights_returns_its_own_code():
    ctx = L.Context(0)
    a = torch.from_numpy(DM.noise(16, 16, 1)).cuda()
    out = torch.full((2,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_DISTS, 1, 16, 16)
    ws = torch.full((need,), CANARY, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.ir_dists(ctx.h, ctx.stream(), L.ptr(a), 16, 48, L.ptr(a), 16, 48, 1, 16, 16, L.ptr(out), None, L.ptr(ws), need)
    assert rc == L.DISTS_NOT_CONFIGURED == -14 and rc not in (L.LPIPS_NOT_CONFIGURED, L.CLIPIQA_NOT_CONFIGURED)
    assert b"not configured" in ctx.lib.ir_last_error(ctx.h)
    # a missing tensor and one of another shape are named
    assert ctx.lib.ir_dists_configure(ctx.h) == -2 and b"dists.c1.w" in ctx.lib.ir_last_error(ctx.h)
    for k, v in DM.weights().items():
        ctx.upload(k, v[:-1] if k == "dists.beta" else v)
    assert ctx.lib.ir_dists_configure(ctx.h) == -2 and b"dists.beta" in ctx.lib.ir_last_error(ctx.h)
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- host layer, pipeline
def _files(d, kind="normal"):
    """The three weight-file forms -> {form: (model file, vgg file or None)}."""
    os.makedirs(d, exist_ok=True)
    w = DM.weights(kind)
    out = {}
    for form in ("module", "vgg"):
        ab, vgg = DM.state_dicts(w, form)
        torch.save(ab, d / f"{form}.pth")
        if vgg is not None:
            torch.save(vgg, d / "vgg16.pth")
        out[form] = (str(d / f"{form}.pth"), str(d / "vgg16.pth") if vgg is not None else None)
    np.savez(d / "dists.npz", **{k: v.numpy() for k, v in w.items()})
    out["npz"] = (str(d / "dists.npz"), None)
    return out


def test_dists_arrays_from_each_weight_file_form(tmp_path):
    from instarevive_amd import dists as DD
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    _bound.clear()
    a, b = DM.pair("35x67_noise")
    got = []
    for form, (model, vgg) in _files(tmp_path).items():
        DD.configure(ctx, model, vgg)
        got.append(DD.dists_arrays(ctx, a, b))
    assert got[0] == got[1] == got[2] == _device_value("35x67_noise")[0]
    with pytest.raises(DD.DistsError):
        DD.dists_arrays(ctx, a[:15], b[:15])


def test_process_returns_what_a_standalone_call_returns(tmp_path):
    """process(..., gt=, dists=True) on the reduced models: the last value of every score is ir_dists of the returned image against its ground
    truth, the values in front are what gt= alone gives, and without dists= the return value is the pair form."""
    from instarevive_amd import dists as DD
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support.metrics_model import ramp
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    _bound.clear()
    model, _ = _files(tmp_path)["module"]
    DD.configure(dit.ctx, model)
    batch = [(det_input(500 + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    gts = [ramp(64, 128, 40), ramp(40, 100, 41)]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    preds, st1, (sp, s1) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=True, gt=gts, **kw)
    assert all(len(s) == 2 for s in sp + s1)
    preds3, st13, (sp3, s13) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=True, gt=gts, dists=True, **kw)
    assert all(np.array_equal(x, z) for x, z in zip(preds + st1, preds3 + st13))
    assert all(len(s) == 3 for s in sp3 + s13)
    assert [s[:2] for s in sp3 + s13] == [tuple(s) for s in sp + s1]
    for arr, g, s in zip(preds3 + st13, gts + gts, sp3 + s13):
        alone = DD.dists_arrays(dit.ctx, arr[:g.shape[0], :g.shape[1]], g)
        assert s[2] == alone and 0 < alone < 1, (s, alone)
    # the stream form, a batch without ground truth in between
    out = list(process_stream(dit, [batch, batch], "wavelet", False, False, 64, 32, gt=[None, gts], dists=True, **kw))
    assert len(out[0]) == 2 and out[1][2][0] == sp3
    with pytest.raises(ValueError, match="dists.*gt"):
        process(dit, batch, 1, "wavelet", False, False, 64, 32, dists=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_dists_model_adds_the_last_column(tmp_path):
    """inference.py --gt --dists_model --dists_vgg --png_encoder gpu --resize gpu over the 17-file folder of tests/test_metrics_gpu.py: metrics.csv
    ends with the column `dists`, ir_dists of the decoded saved PNG against its ground truth, and the averages end with the `dists:` line."""
    from instarevive_amd import dists as DD
    from instarevive_amd.metrics import read_report
    from instarevive_amd.models import get_context
    from tests.test_metrics_gpu import _cli_folder, _run
    d = tmp_path
    truth, cmd = _cli_folder(d)
    model, vgg = _files(d / "w")["vgg"]
    stdout = _run(cmd + ["--png_encoder", "gpu", "--resize", "gpu", "--output", str(d / "out"), "--dists_model", model, "--dists_vgg", vgg])
    assert "were not scored" not in stdout and "--gt: scored 17 files" in stdout, stdout[-1500:]
    lines = (d / "out" / "metrics.csv").read_text().splitlines()
    assert lines[0] == "file,psnr_y,ssim_y,dists" and len(lines) == 18 and all(len(ln.split(",")) == 4 for ln in lines)
    ctx = get_context(torch.device("cuda", 0))
    _bound.clear()
    DD.configure(ctx, model, vgg)
    got = read_report(str(d / "out" / "metrics.csv"))
    for k, g in truth.items():
        saved = np.array(Image.open(d / "out" / k).convert("RGB"))
        assert got[k][2] == DD.dists_arrays(ctx, saved, g), k
    avg = [ln for ln in stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ", "dists: "))]
    assert [ln.split(":")[0] for ln in avg] == ["psnr", "ssim", "dists"]
    assert avg[2] == f"dists: {np.mean([v[2] for v in got.values()]):.5f}"


def test_eval_batch_and_evaluate_pairs_take_the_flag(tmp_path):
    """eval_batch.py --gt --dists_model: both reports end with the `dists` column, ir_dists of the saved file against the cropped ground truth;
    tools/evaluate_pairs.py --backend gpu --dists_model prints the mean of ir_dists over a folder as its last line."""
    from instarevive_amd import dists as DD
    from instarevive_amd.metrics import read_report
    from instarevive_amd.models import get_context
    from instarevive_amd.utils import center_crop_arr
    from tests.golden._det import det_input
    from tests.support.metrics_model import ramp
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_metrics_gpu import _run
    d = tmp_path
    _write_artifacts(d)
    model, _ = _files(d / "w")["npz"]
    os.makedirs(d / "lq")
    os.makedirs(d / "gt")
    truth = {}
    for i, (k, hw) in enumerate({"a.png": (70, 90), "b.png": (64, 100)}.items()):
        Image.fromarray((det_input(80 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "lq" / k)
        Image.fromarray(ramp(hw[0] + 9, hw[1] + 5, 30 + i)).save(d / "gt" / k)
        truth[k] = np.ascontiguousarray(center_crop_arr(Image.open(d / "gt" / k).convert("RGB"), 64))
    stdout = _run([sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "lq"), "--output",
                   str(d / "res"), "--cond_output", str(d / "cond"), "--batch_size", "2", "--image_size", "64", "--swinir_ckpt",
                   str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
                   "--prompt_embeds", str(d / "prompt.pth"), "--gt", str(d / "gt"), "--dists_model", model])
    ctx = get_context(torch.device("cuda", 0))
    _bound.clear()
    DD.configure(ctx, model)
    for folder in ("res", "cond"):
        assert (d / folder / "metrics.csv").read_text().splitlines()[0] == "file,psnr_y,ssim_y,dists"
        got = read_report(str(d / folder / "metrics.csv"))
        assert sorted(got) == sorted(truth)
        for k, g in truth.items():
            assert got[k][2] == DD.dists_arrays(ctx, np.array(Image.open(d / folder / k).convert("RGB")), g), (folder, k)
    assert len([ln for ln in stdout.splitlines() if ln.startswith("dists: ")]) == 2 and "were not scored" not in stdout
    # evaluate_pairs over the saved folder against the cropped ground truth
    os.makedirs(d / "crop")
    for k, g in truth.items():
        Image.fromarray(g).save(d / "crop" / k)
    stdout = _run([sys.executable, os.path.join(ROOT, "tools", "evaluate_pairs.py"), "-i", str(d / "res"), "-r", str(d / "crop"), "--backend", "gpu", "--dists_model", model])
    want = np.mean([got_k[2] for got_k in read_report(str(d / "res" / "metrics.csv")).values()])
    assert stdout.splitlines()[-1] == f"dists: {want:.5f}", stdout[-500:]
