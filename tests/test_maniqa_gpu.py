"""ir_maniqa (csrc/maniqa.hip) through the C ABI, the pipeline and the command line against the float64 model, tools/evaluate_maniqa.py.

The gate (tests/support/maniqa_model.py): the score within GATE_FACTOR x the fp32 CPU model's largest absolute deviation from the float64
model over the cases, the head-input tokens within GATE_FACTOR x its largest relative L2 deviation. tests/test_maniqa_cpu.py shows that every
planted bug misses this gate by more than ten times. No test provokes a fault: origins outside the image are only shown to be refused by the
Python layer."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import maniqa_model as MM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
NAMES = [c[0] for c in MM.CASES]


def _ctx(kind="small"):
    """The shared context with the seeded model `kind` bound (re-bound only when the other one was)."""
    from instarevive_amd import maniqa
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if ctx.__dict__.get("_test_maniqa_kind") != kind:
        maniqa.configure(ctx, MM.model(kind))
        ctx.__dict__["_test_maniqa_kind"] = kind
    return ctx


def _per_crop(kind):
    cfg = MM.CONFIGS[kind]
    return (cfg["crop"] // cfg["patch"]) ** 2 * (cfg["embed"] // 2)


def _call(buf: np.ndarray, h: int, w: int, origins, kind="small", per_pass=0):
    """ir_maniqa on buf [n][rows][pitch] (bytes) at origins [n][crops][2] with exactly the workspace reported for passes of per_pass crops (0: one)
    -> (scores [n], feat [n][crops * tokens * embed / 2]). scores and feat have canary values behind them and the workspace 16 canary bytes
    behind its stated size: all must stay untouched."""
    ctx = _ctx(kind)
    n, rows, pitch = buf.shape
    org = np.ascontiguousarray(np.asarray(origins, np.int32).reshape(n, -1, 2))
    crops, per = org.shape[1], _per_crop(kind)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    dorg = torch.from_numpy(org).cuda()
    scores = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    feat = torch.full((n * crops * per + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_MANIQA, n, 0, 0, crops, per_pass)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_maniqa(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(dorg), crops, L.ptr(scores), L.ptr(feat), L.ptr(ws), need), "ir_maniqa")
    torch.cuda.synchronize()
    s, f = scores.cpu().numpy(), feat.cpu().numpy()
    assert np.all(s[n:] == OUT_CANARY), "values behind scores were written"
    assert np.all(f[n * crops * per:] == OUT_CANARY), "values behind feat were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return s[:n].copy(), f[:n * crops * per].reshape(n, -1).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


@pytest.fixture(scope="module")
def device_results():
    """{case: (score, feat)} of every case, one call each with the least workspace; computed once (the cases of one model together)."""
    out = {}
    for name, h, w, kind, _, _ in sorted(MM.CASES, key=lambda c: c[3]):
        s, f = _call(_tight([MM.image(name)]), h, w, [MM.origins(name)], kind)
        out[name] = (s[0], f[0])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_score_and_tokens_are_within_the_gate_of_the_float64_model(name, device_results):
    score, feat = device_results[name]
    ds, df = MM.deviations(score, feat, name)
    gs, gf = MM.gate()
    print(f"{name}: maniqa {score:.12f} (model {MM.reference(name)[0]:.12f}); score deviation {ds:.3e} (gate {gs:.3e}), token deviation {df:.3e} (gate {gf:.3e}); "
          f"host fp32 {MM.host_deviation(name)[0]:.3e} / {MM.host_deviation(name)[1]:.3e}")
    assert np.isfinite(score) and ds <= gs
    assert df <= gf


def test_the_same_case_twice_gives_the_same_bits_and_a_batch_each_image_its_own(device_results):
    name = "70x131"
    img, org = MM.image(name), MM.origins(name)
    s, f = _call(_tight([img]), 70, 131, [org])
    assert _same(s[0], device_results[name][0]) and _same(f[0], device_results[name][1])
    other = MM.ramp(70, 131, 5)
    other_org = [(y // 2, x // 3) for y, x in org]
    sb, fb = _call(_tight([img, other, img]), 70, 131, [org, other_org, org], per_pass=4)   # passes of 4 crops cross the images' borders
    assert _same(sb[0], s[0]) and _same(fb[0], f[0])
    assert _same(sb[2], s[0]) and _same(fb[2], f[0])
    so, fo = _call(_tight([other]), 70, 131, [other_org])
    assert _same(sb[1], so[0]) and _same(fb[1], fo[0]) and sb[0] != sb[1]


def test_one_pass_and_one_crop_per_pass_give_the_same_bits(device_results):
    """The 20-crop case with the workspace of one crop per pass (device_results), of 7 per pass (three passes, the last one short) and of all
    crops at once."""
    name = "100x200"
    for per_pass in (7, 20):
        s, f = _call(_tight([MM.image(name)]), 100, 200, [MM.origins(name)], per_pass=per_pass)
        assert _same(s[0], device_results[name][0]) and _same(f[0], device_results[name][1])


def test_embedded_image_with_rows_and_pitch(device_results):
    """rows > h and pitch > 3 w: the same bits as the tight image."""
    name = "97x83"
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1, 104, 3 * 83 + 37), dtype=np.uint8)
    buf[0, :97, :3 * 83] = MM.image(name).reshape(97, -1)
    s, f = _call(buf, 97, 83, [MM.origins(name)])
    assert _same(s[0], device_results[name][0]) and _same(f[0], device_results[name][1])


def test_bad_arguments_are_refused_and_write_nothing(device_results):
    ctx = _ctx()
    name, h, w = "65x65", 65, 65
    img = torch.from_numpy(MM.image(name)).cuda()
    org = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    out = torch.full((1 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_MANIQA, 1, 0, 0, 5, 0)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, crops=5, pi=L.ptr(img), pg=L.ptr(org), po=L.ptr(out), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_maniqa(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, pg, crops, po, None, pw, wsb)

    assert call(n=0) == -1 and call(crops=0) == -1 and call(hh=0, rows=1) == -1 and call(ww=0) == -1
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    assert call(hh=64, ww=65) == -1 and "64 x 65" in ctx.lib.ir_last_error(ctx.h).decode()     # the short side is not above the crop
    assert ctx.ws_bytes(L.STAGE_MANIQA, 0, 0, 0, 5, 0) == 0 and ctx.ws_bytes(L.STAGE_MANIQA, 1, 0, 0, 0, 0) == 0
    assert ctx.ws_bytes(L.STAGE_MANIQA, 1, 999, 7, 5, 0) == need                                 # h x w does not matter
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(po=C.c_void_p(out.data_ptr() + 4)) == -1                  # misaligned scores
    assert call(pi=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(pg=None) == -1 and call(handle=None) == -1
    # a context that was never configured: the documented code, and no workspace size
    fresh = L.Context(0)
    assert fresh.ws_bytes(L.STAGE_MANIQA, 1, 0, 0, 5, 0) == 0
    assert call(handle=fresh.h) == L.MANIQA_NOT_CONFIGURED
    assert "not configured" in fresh.lib.ir_last_error(fresh.h).decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0                                                    # feat may be NULL
    torch.cuda.synchronize()
    assert _same(out[:1].cpu().numpy()[0], device_results[name][0])


def test_configure_names_a_missing_or_misshapen_tensor():
    from instarevive_amd import maniqa
    fresh = L.Context(0)
    m = MM.model("small")
    cfg = m["cfg"]
    taps = (C.c_int * 4)(*cfg["taps"])

    def conf(crop=64, embed=64, swin_heads=2, tp=taps):
        return fresh.lib.ir_maniqa_configure(fresh.h, crop, 8, embed, 2, 256, 5, tp, 4, swin_heads, 2, 64, C.c_float(0.8))

    assert conf() == -2 and "maniqa." in fresh.lib.ir_last_error(fresh.h).decode()
    assert conf(crop=60) == -1 and conf(embed=96) == -1 and conf(swin_heads=5) == -1 and "unsupported" in fresh.lib.ir_last_error(fresh.h).decode()
    assert conf(tp=(C.c_int * 4)(1, 2, 3, 5)) == -1 and conf(tp=(C.c_int * 4)(1, 3, 2, 4)) == -1
    maniqa.configure(fresh, m)
    fresh.upload("maniqa.swin2.1.1.attn.rpb", torch.zeros(7))
    assert conf() == -2 and "maniqa.swin2.1.1.attn.rpb" in fresh.lib.ir_last_error(fresh.h).decode()


def test_score_arrays_checks_the_origins_and_gives_the_calls_bits(device_results, monkeypatch):
    from instarevive_amd import maniqa
    ctx = _ctx()
    name = "70x131"
    img = MM.image(name)
    assert maniqa.score_arrays(ctx, img) == device_results[name][0]                         # the uniform grid is the default
    assert maniqa.score_arrays(ctx, MM.image("97x83"), MM.origins("97x83")) == device_results["97x83"][0]
    with pytest.raises(ValueError, match="64 x 200"):
        maniqa.score_arrays(ctx, MM.ramp(64, 200, 1))
    for bad in ([(7, 0)], [(0, 68)], [(-1, 0)]):                                           # refused on the host: nothing is uploaded, nothing runs
        with pytest.raises(ValueError, match="origin"):
            maniqa.score_arrays(ctx, img, bad)
    # a cap below two crops' workspace: one crop per pass, the same bits
    monkeypatch.setattr(maniqa, "WS_CAP", maniqa.ws_bytes(ctx, 1, 5, 1))
    assert maniqa.crops_per_pass(ctx, 1, 5) == 1
    assert maniqa.score_arrays(ctx, img) == device_results[name][0]


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _model_score(arr, origins=None):
    """The float64 model's score of an array, NaN where it has none."""
    try:
        return MM.EM.maniqa(arr, MM.model("small"), origins, torch.float64)
    except MM.EM.ManiqaError:
        return float("nan")


def test_process_scores_the_returned_images():
    """process(maniqa=True) on the reduced models: the extra element holds the kernel's score of the image the same call returns, in the last place
    of every tuple - alone and with gt=, whose rectangle it then scores; a rectangle with a short side of 64 or less gets NaN."""
    from instarevive_amd import maniqa
    from instarevive_amd.pipeline import process
    from tests.golden._det import det_input
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    ctx = _ctx()
    assert dit.ctx is ctx
    batch = [(det_input(720 + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    gate = MM.gate()[0]
    preds, _, (sp, _) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, maniqa=True, **kw)
    assert all(len(t) == 1 for t in sp)
    for (v,), p in zip(sp, preds):
        want = _model_score(p)
        print(f"192 x 256: maniqa {v:.12f} (model {want:.12f})")
        assert abs(v - want) <= gate and v == maniqa.score_arrays(ctx, p)
    assert len(process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, **kw)) == 2
    gts = [MM.ramp(192, 200, 1), MM.ramp(64, 256, 2)]
    p2, _, (sg, _) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, maniqa=True, **kw)
    assert all(len(t) == 3 for t in sg) and abs(sg[0][2] - _model_score(p2[0][:192, :200])) <= gate and np.isnan(sg[1][2])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_maniqa_model_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --maniqa_model --maniqa_crops random --gt over three small PNGs: metrics.csv holds `file,psnr_y,ssim_y,maniqa` rows whose last
    value is within the gate of the float64 model's score of the DECODED SAVED PNG at the origins tools/evaluate_maniqa.py draws for that file,
    and the printed average is the one that tool prints for the folder."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in")
    os.makedirs(d / "gt")
    for i, hw in enumerate([(72, 80), (96, 80), (128, 66)]):
        Image.fromarray((det_input(860 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / f"im{i}.png")
        Image.fromarray(MM.ramp(hw[0], hw[1], 30 + i)).save(d / "gt" / f"im{i}.png")
    MM.EM.save_npz(d / "maniqa.npz", MM.model("small"))
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--maniqa_model", str(d / "maniqa.npz"), "--maniqa_crops", "random",
           "--maniqa_seed", "9", "--gt", str(d / "gt"), "--output", str(d / "out"), "--png_encoder", "gpu", "--resize", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = (d / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,psnr_y,ssim_y,maniqa"
    got = read_report(str(d / "out" / "metrics.csv"))
    assert sorted(got) == ["im0_0.png", "im1_0.png", "im2_0.png"]
    gate = MM.gate()[0]
    for k in got:
        arr = np.array(Image.open(d / "out" / k).convert("RGB"))
        want = _model_score(arr, MM.EM.crop_origins(arr.shape[0], arr.shape[1], 64, 5, "random", 9, k))
        print(f"{k}: maniqa {got[k][2]:.12f} (model {want:.12f})")
        assert abs(got[k][2] - want) <= gate, (k, got[k], want)
    assert "were not scored" not in r.stdout and "--gt / --maniqa_model: scored 3 files" in r.stdout, r.stdout[-1500:]
    assert f"maniqa: {np.mean([v[2] for v in got.values()]):.5f}" in r.stdout.splitlines()
    lines = []
    avg = MM.EM.evaluate(str(d / "out"), str(d / "maniqa.npz"), mode="random", seed=9, log=lines.append)
    assert abs(avg - np.mean([v[2] for v in got.values()])) <= gate and lines[-1].startswith("maniqa: ")
