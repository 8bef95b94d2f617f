"""ir_clipiqa (csrc/clipiqa.hip) through the C ABI, the pipeline and the command line against the float64 model, tools/evaluate_clipiqa.py.

The gate (tests/support/clipiqa_model.py): the score within GATE_FACTOR x the fp32 CPU model's largest absolute deviation from the float64
model over the cases, the feature vector within GATE_FACTOR x its largest relative L2 deviation. tests/test_clipiqa_cpu.py shows that every
planted bug misses this gate by more than ten times."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import clipiqa_model as CM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
NAMES = [c[0] for c in CM.CASES]


def _ctx(kind="small"):
    """The shared context with the seeded model `kind` bound (re-bound only when the other one was)."""
    from instarevive_amd import clipiqa
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if ctx.__dict__.get("_test_clipiqa_kind") != kind:
        clipiqa.configure(ctx, CM.model(kind))
        ctx.__dict__["_test_clipiqa_kind"] = kind
    return ctx


def _call(buf: np.ndarray, h: int, w: int, kind="small"):
    """ir_clipiqa on buf [n][rows][pitch] (bytes) with exactly the reported workspace -> (scores [n], feat [n][OUT_DIM]). scores and feat have
    canary values behind them and the workspace 16 canary bytes behind its stated size: all must stay untouched."""
    ctx = _ctx(kind)
    n, rows, pitch = buf.shape
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    scores = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    feat = torch.full((n * CM.OUT_DIM + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_CLIPIQA, n, h, w)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_clipiqa(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(scores), L.ptr(feat), L.ptr(ws), need), "ir_clipiqa")
    torch.cuda.synchronize()
    s, f = scores.cpu().numpy(), feat.cpu().numpy()
    assert np.all(s[n:] == OUT_CANARY), "values behind scores were written"
    assert np.all(f[n * CM.OUT_DIM:] == OUT_CANARY), "values behind feat were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return s[:n].copy(), f[:n * CM.OUT_DIM].reshape(n, CM.OUT_DIM).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def device_results():
    """{case: (score, feat [OUT_DIM])} of every case, one call each; computed once (the cases of one model together: a re-bind per model)."""
    out = {}
    for name, h, w, kind in sorted(CM.CASES, key=lambda c: c[3]):
        s, f = _call(_tight([CM.image(name)]), h, w, kind)
        out[name] = (s[0], f[0])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_score_and_feature_are_within_the_gate_of_the_float64_model(name, device_results):
    score, feat = device_results[name]
    ds, df = CM.deviations(score, feat, name)
    gs, gf = CM.gate()
    print(f"{name}: clipiqa {score:.12f} (model {CM.reference(name)[0]:.12f}); score deviation {ds:.3e} (gate {gs:.3e}), feature deviation {df:.3e} (gate {gf:.3e})")
    assert np.isfinite(score) and ds <= gs
    assert df <= gf


def test_the_same_case_twice_gives_the_same_bits_and_a_batch_each_image_its_own(device_results):
    name = "70x45"
    img = CM.image(name)
    s, f = _call(_tight([img]), 70, 45)
    assert np.array_equal(_bits(s), _bits(np.array([device_results[name][0]]))) and np.array_equal(_bits(f[0]), _bits(device_results[name][1]))
    other = CM.ramp(70, 45, 5)
    sb, fb = _call(_tight([other, img, other]), 70, 45)
    assert _bits(sb[1:2])[0] == _bits(s)[0] and np.array_equal(_bits(fb[1]), _bits(f[0]))
    assert _bits(sb[0:1])[0] == _bits(sb[2:3])[0] and np.array_equal(_bits(fb[0]), _bits(fb[2]))
    assert sb[0] != sb[1]


def test_embedded_image_with_rows_and_pitch(device_results):
    """rows > h and pitch > 3 w: the same bits as the tight image."""
    name = "63x95"
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1, 70, 3 * 95 + 37), dtype=np.uint8)
    buf[0, :63, :3 * 95] = CM.image(name).reshape(63, -1)
    s, f = _call(buf, 63, 95)
    assert _bits(s)[0] == _bits(np.array([device_results[name][0]]))[0] and np.array_equal(_bits(f[0]), _bits(device_results[name][1]))


def test_bad_arguments_are_refused_and_write_nothing(device_results):
    from instarevive_amd.models import get_context
    ctx = _ctx()
    h, w = 32, 32
    img = torch.from_numpy(CM.image("32x32")).cuda()
    out = torch.full((1 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_CLIPIQA, 1, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(img), po=L.ptr(out), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_clipiqa(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, po, None, pw, wsb)

    assert call(n=0) == -1 and call(hh=31, rows=31) == -1 and call(ww=31) == -1
    assert "32 x 32" in ctx.lib.ir_last_error(ctx.h).decode()
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(pi=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    assert ctx.ws_bytes(L.STAGE_CLIPIQA, 1, 31, 64) == 0
    # a context that was never configured: the documented code, and no workspace size
    fresh = L.Context(0)
    assert fresh.ws_bytes(L.STAGE_CLIPIQA, 1, h, w) == 0
    assert call(handle=fresh.h) == L.CLIPIQA_NOT_CONFIGURED
    assert "not configured" in fresh.lib.ir_last_error(fresh.h).decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0                                                    # feat may be NULL
    torch.cuda.synchronize()
    assert _bits(out[:1].cpu().numpy())[0] == _bits(np.array([device_results["32x32"][0]]))[0]


def test_configure_names_a_missing_or_misshapen_tensor():
    fresh = L.Context(0)
    m = CM.model("small")
    layers = (C.c_int * 4)(*m["cfg"]["layers"])

    def conf():
        return fresh.lib.ir_clipiqa_configure(fresh.h, layers, CM.WIDTH, 32, CM.OUT_DIM, CM.PAIRS, C.c_float(100.0))

    assert conf() == -2 and "clipiqa.conv1.weight" in fresh.lib.ir_last_error(fresh.h).decode()
    from instarevive_amd import clipiqa
    clipiqa.configure(fresh, m)
    fresh.upload("clipiqa.layer2.0.downsample.1.running_var", torch.zeros(7))
    assert conf() == -2 and "clipiqa.layer2.0.downsample.1.running_var" in fresh.lib.ir_last_error(fresh.h).decode()


def test_score_arrays_and_a_split_batch_give_the_calls_bits(device_results, monkeypatch):
    from instarevive_amd import clipiqa
    ctx = _ctx()
    img = CM.image("97x130")
    assert clipiqa.score_arrays(ctx, img) == device_results["97x130"][0]
    with pytest.raises(ValueError):
        clipiqa.score_arrays(ctx, CM.ramp(31, 200, 1))
    # a cap below two images' workspace: three images go out one per call, with the bits of one call
    dev = torch.from_numpy(np.stack([img, CM.ramp(97, 130, 3), img])).cuda()
    whole = clipiqa.queue_clipiqa(ctx, dev.data_ptr(), 97, 3 * 130, 3, 97, 130).clone()
    monkeypatch.setattr(clipiqa, "WS_CAP", clipiqa.ws_bytes(ctx, 1, 97, 130))
    assert clipiqa.images_per_call(ctx, 3, 97, 130) == 1
    clipiqa.queue_clipiqa(ctx, dev.data_ptr(), 97, 3 * 130, 3, 97, 130)
    split = clipiqa.fetch_clipiqa(ctx, 3)
    assert split == whole.cpu().tolist() and split[0] == split[2] == device_results["97x130"][0]


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _model_score(arr):
    """The float64 model's score of an array, NaN where it has none."""
    if min(arr.shape[:2]) < 32:
        return float("nan")
    return CM.EC.clipiqa(arr, CM.model("small"), torch.float64)


def _assert_clipiqa(values, arrays):
    assert len(values) == len(arrays)
    gate = CM.gate()[0]
    for v, arr in zip(values, arrays):
        want = _model_score(arr)
        print(f"{arr.shape[0]} x {arr.shape[1]}: clipiqa {v:.12f} (model {want:.12f})")
        assert (np.isnan(v) and np.isnan(want)) or abs(v - want) <= gate, (v, want)


def test_process_and_process_stream_score_the_returned_images():
    """process(clipiqa=True) and process_stream(clipiqa=True) on the reduced models: the extra element holds the kernel's score of the image the
    same call returns, in the last place of every tuple - alone, with gt= and with niqe=; a batch whose niqe_rects entry is None is not scored."""
    from instarevive_amd import clipiqa
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support import niqe_model as NM
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    ctx = _ctx()
    assert dit.ctx is ctx
    batches = [[(det_input(820 + 2 * b + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    # alone: a pair of lists of (clipiqa,), the kernel's own value of the returned image
    preds, st1, (sp, s1) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=True, clipiqa=True, **kw)
    assert all(len(t) == 1 for t in sp + s1)
    _assert_clipiqa([t[0] for t in sp], preds)
    _assert_clipiqa([t[0] for t in s1], st1)
    assert [t[0] for t in sp] == [clipiqa.score_arrays(ctx, p) for p in preds]
    assert len(process(dit, batches[0], 1, "wavelet", False, False, 64, 32, **kw)) == 2
    # with gt=: the value is appended to each tuple, and the rectangle is the ground truth's (31 pixels: no score)
    gts = [CM.ramp(192, 200, 1), CM.ramp(31, 256, 2)]
    p2, _, (sg, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, clipiqa=True, **kw)
    assert all(len(t) == 3 for t in sg) and all(np.array_equal(a, b) for a, b in zip(p2, preds))
    _assert_clipiqa([t[2] for t in sg], [p[:g.shape[0], :g.shape[1]] for p, g in zip(p2, gts)])
    assert np.isnan(sg[1][2])
    assert [t[:2] for t in sg] == process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, **kw)[2][0]
    # with niqe=: (niqe, clipiqa), NIQE's value unchanged
    _, _, (sn, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, niqe=NM.params(), clipiqa=True, **kw)
    only = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, niqe=NM.params(), **kw)[2][0]
    assert all(len(t) == 2 for t in sn) and [t[:1] for t in sn] == only and [t[1] for t in sn] == [t[0] for t in sp]
    # process_stream(): niqe_rects in step with the batches; the second batch is not scored
    rects = [[(192, 200), (96, 256)], None]
    out = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, clipiqa=True, niqe_rects=rects, **kw))
    assert [len(r) for r in out] == [3, 2]
    _assert_clipiqa([t[0] for t in out[0][2][0]], [a[:r[0], :r[1]] for a, r in zip(out[0][0], rects[0])])
    _assert_clipiqa([t[0] for t in out[0][2][1]], [a[:r[0], :r[1]] for a, r in zip(out[0][1], rects[0])])
    every = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=False, clipiqa=True, **kw))
    assert [t[0] for t in every[0][2][0]] == [t[0] for t in sp]
    _assert_clipiqa([t[0] for t in every[1][2][0]], every[1][0])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_clipiqa_model_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --clipiqa_model (an .npz that carries the text rows) without --gt, --png_encoder gpu --resize gpu: metrics.csv holds
    `file,clipiqa` rows that are within the gate of the float64 model's score of the DECODED SAVED PNG, and the average line is their mean."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep")
    for i, hw in enumerate([(64, 64), (96, 80)]):
        Image.fromarray((det_input(960 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / ("deep/" if i == 1 else "") / f"im{i}.png")
    m = CM.model("small")
    np.savez(d / "rn50.npz", text=m["text"].numpy(), **{k: v.numpy() for k, v in m["sd"].items()})
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--clipiqa_model", str(d / "rn50.npz"),
           "--output", str(d / "out"), "--png_encoder", "gpu", "--resize", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = (d / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,clipiqa"
    got = read_report(str(d / "out" / "metrics.csv"))
    assert sorted(got) == ["deep/im1_0.png", "im0_0.png"]
    gate = CM.gate()[0]
    for k in got:
        want = _model_score(np.array(Image.open(d / "out" / k).convert("RGB")))
        print(f"{k}: clipiqa {got[k][0]:.12f} (model {want:.12f})")
        assert abs(got[k][0] - want) <= gate, (k, got[k], want)
    assert "were not scored" not in r.stdout and "--clipiqa_model: scored 2 files" in r.stdout, r.stdout[-1500:]
    assert f"clipiqa: {np.mean([v[0] for v in got.values()]):.5f}" in r.stdout.splitlines()
