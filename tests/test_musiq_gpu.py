"""ir_musiq (csrc/musiq.hip) through the C ABI, the pipeline and the command line against the float64 model, tools/evaluate_musiq.py.

The gate (tests/support/musiq_model.py): the score within GATE_FACTOR x the fp32 CPU model's largest absolute deviation from the float64
model over the cases, the class-token feature within GATE_FACTOR x its largest relative L2 deviation. tests/test_musiq_cpu.py shows that every
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
from tests.support import musiq_model as MM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
NAMES = [c[0] for c in MM.CASES]
HID = MM.HIDDEN


def _ctx(kind="small"):
    """The shared context with the seeded model `kind` bound (re-bound only when the other one was)."""
    from instarevive_amd import musiq
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if ctx.__dict__.get("_test_musiq_kind") != kind:
        musiq.configure(ctx, MM.model(kind))
        ctx.__dict__["_test_musiq_kind"] = kind
    return ctx


def _call(buf: np.ndarray, h: int, w: int, kind="small"):
    """ir_musiq on buf [n][rows][pitch] (bytes) with exactly the reported workspace -> (scores [n], feat [n][HID]). scores and feat have canary
    values behind them and the workspace 16 canary bytes behind its stated size: all must stay untouched."""
    ctx = _ctx(kind)
    n, rows, pitch = buf.shape
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    scores = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    feat = torch.full((n * HID + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_MUSIQ, n, h, w)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_musiq(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(scores), L.ptr(feat), L.ptr(ws), need), "ir_musiq")
    torch.cuda.synchronize()
    s, f = scores.cpu().numpy(), feat.cpu().numpy()
    assert np.all(s[n:] == OUT_CANARY), "values behind scores were written"
    assert np.all(f[n * HID:] == OUT_CANARY), "values behind feat were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return s[:n].copy(), f[:n * HID].reshape(n, HID).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def device_results():
    """{case: (score, feat [HID])} of every case, one call each; computed once (the cases of one model together: a re-bind per model)."""
    out = {}
    for name, h, w, kind in sorted(MM.CASES, key=lambda c: c[3]):
        s, f = _call(_tight([MM.image(name)]), h, w, kind)
        out[name] = (s[0], f[0])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_score_and_feature_are_within_the_gate_of_the_float64_model(name, device_results):
    score, feat = device_results[name]
    ds, df = MM.deviations(score, feat, name)
    gs, gf = MM.gate()
    print(f"{name}: musiq {score:.12f} (model {MM.reference(name)[0]:.12f}); score deviation {ds:.3e} (gate {gs:.3e}), feature deviation {df:.3e} (gate {gf:.3e})")
    assert np.isfinite(score) and ds <= gs
    assert df <= gf


def test_the_same_case_twice_gives_the_same_bits_and_a_batch_each_image_its_own(device_results):
    name = "33x70"
    img = MM.image(name)
    s, f = _call(_tight([img]), 33, 70)
    assert np.array_equal(_bits(s), _bits(np.array([device_results[name][0]]))) and np.array_equal(_bits(f[0]), _bits(device_results[name][1]))
    other = MM.ramp(33, 70, 5)
    sb, fb = _call(_tight([img, other, img]), 33, 70)
    assert _bits(sb[0:1])[0] == _bits(s)[0] and np.array_equal(_bits(fb[0]), _bits(f[0]))
    assert _bits(sb[2:3])[0] == _bits(s)[0] and np.array_equal(_bits(fb[2]), _bits(f[0]))
    so, fo = _call(_tight([other]), 33, 70)
    assert _bits(sb[1:2])[0] == _bits(so)[0] and np.array_equal(_bits(fb[1]), _bits(fo[0])) and sb[0] != sb[1]


def test_embedded_image_with_rows_and_pitch(device_results):
    """rows > h and pitch > 3 w: the same bits as the tight image."""
    name = "45x97"
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1, 52, 3 * 97 + 37), dtype=np.uint8)
    buf[0, :45, :3 * 97] = MM.image(name).reshape(45, -1)
    s, f = _call(buf, 45, 97)
    assert _bits(s)[0] == _bits(np.array([device_results[name][0]]))[0] and np.array_equal(_bits(f[0]), _bits(device_results[name][1]))


def test_bad_arguments_are_refused_and_write_nothing(device_results):
    ctx = _ctx()
    h, w = 32, 32
    img = torch.from_numpy(MM.image("32x32")).cuda()
    out = torch.full((1 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_MUSIQ, 1, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(img), po=L.ptr(out), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_musiq(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, po, None, pw, wsb)

    assert call(n=0) == -1 and call(hh=0, rows=1) == -1 and call(ww=0) == -1
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    # a resized side rounds to 0: refused, the size named, no workspace size
    sliver = torch.zeros((1, 1000, 3), dtype=torch.uint8, device="cuda")
    assert call(hh=1, ww=1000, rows=1, pitch=3000, pi=L.ptr(sliver)) == -1 and "1 x 1000" in ctx.lib.ir_last_error(ctx.h).decode()
    assert ctx.ws_bytes(L.STAGE_MUSIQ, 1, 1, 1000) == 0 and ctx.ws_bytes(L.STAGE_MUSIQ, 0, 32, 32) == 0
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(po=C.c_void_p(out.data_ptr() + 4)) == -1                  # misaligned scores
    assert call(pi=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    # a context that was never configured: the documented code, and no workspace size
    fresh = L.Context(0)
    assert fresh.ws_bytes(L.STAGE_MUSIQ, 1, h, w) == 0
    assert call(handle=fresh.h) == L.MUSIQ_NOT_CONFIGURED
    assert "not configured" in fresh.lib.ir_last_error(fresh.h).decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0                                                    # feat may be NULL
    torch.cuda.synchronize()
    assert _bits(out[:1].cpu().numpy())[0] == _bits(np.array([device_results["32x32"][0]]))[0]


def test_configure_names_a_missing_or_misshapen_tensor():
    from instarevive_amd import musiq
    fresh = L.Context(0)
    m = MM.model("small")
    lon = (C.c_int * 3)(*m["cfg"]["longer"])

    def conf(patch=32, hidden=384, heads=6):
        return fresh.lib.ir_musiq_configure(fresh.h, patch, hidden, 1152, heads, 2, 10, 3, lon)

    assert conf() == -2 and "musiq.stem.conv.weight" in fresh.lib.ir_last_error(fresh.h).decode()
    assert conf(patch=16) == -1 and conf(heads=5) == -1 and "unsupported" in fresh.lib.ir_last_error(fresh.h).decode()
    musiq.configure(fresh, m)
    fresh.upload("musiq.layers.1.mlp.fc2.bias", torch.zeros(7))
    assert conf() == -2 and "musiq.layers.1.mlp.fc2.bias" in fresh.lib.ir_last_error(fresh.h).decode()


def test_score_arrays_and_a_split_batch_give_the_calls_bits(device_results, monkeypatch):
    from instarevive_amd import musiq
    ctx = _ctx()
    img = MM.image("100x131")
    assert musiq.score_arrays(ctx, img) == device_results["100x131"][0]
    with pytest.raises(ValueError, match="1 x 1000"):
        musiq.score_arrays(ctx, MM.ramp(1, 1000, 1))
    # a cap below two images' workspace: three images go out one per call, with the bits of one call
    dev = torch.from_numpy(np.stack([img, MM.ramp(100, 131, 3), img])).cuda()
    whole = musiq.queue_musiq(ctx, dev.data_ptr(), 100, 3 * 131, 3, 100, 131).clone()
    monkeypatch.setattr(musiq, "WS_CAP", musiq.ws_bytes(ctx, 1, 100, 131))
    assert musiq.images_per_call(ctx, 3, 100, 131) == 1
    musiq.queue_musiq(ctx, dev.data_ptr(), 100, 3 * 131, 3, 100, 131)
    split = musiq.fetch_musiq(ctx, 3)
    assert split == whole.cpu().tolist() and split[0] == split[2] == device_results["100x131"][0]


def test_attention_in_several_launches_gives_the_same_bits():
    """The attention of a call runs as many (image, head) pairs per launch as fit its score buffer. 5 images of 300 x 500 (T = 292, 30 pairs) need
    more than one launch; each image keeps the bits of a call of its own, which takes one."""
    imgs = [MM.ramp(300, 500, 40 + i) for i in range(5)]
    sb, fb = _call(_tight(imgs), 300, 500)
    for i in (0, 4):
        s, f = _call(_tight([imgs[i]]), 300, 500)
        assert _bits(sb[i:i + 1])[0] == _bits(s)[0] and np.array_equal(_bits(fb[i]), _bits(f[0]))


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _model_score(arr):
    """The float64 model's score of an array, NaN where it has none."""
    try:
        return MM.EM.musiq(arr, MM.model("small"), torch.float64)
    except MM.EM.MusiqError:
        return float("nan")


def _assert_musiq(values, arrays):
    assert len(values) == len(arrays)
    gate = MM.gate()[0]
    for v, arr in zip(values, arrays):
        want = _model_score(arr)
        print(f"{arr.shape[0]} x {arr.shape[1]}: musiq {v:.12f} (model {want:.12f})")
        assert (np.isnan(v) and np.isnan(want)) or abs(v - want) <= gate, (v, want)


def test_process_and_process_stream_score_the_returned_images():
    """process(musiq=True) and process_stream(musiq=True) on the reduced models: the extra element holds the kernel's score of the image the same
    call returns, in the last place of every tuple - alone, with gt=, with niqe= and clipiqa=; with niqe_rects, a batch whose entry is None is
    not scored. Without musiq the tuples are what they were."""
    from instarevive_amd import clipiqa, musiq
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support import clipiqa_model as CM
    from tests.support import niqe_model as NM
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    ctx = _ctx()
    assert dit.ctx is ctx
    batches = [[(det_input(820 + 2 * b + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    # alone: a pair of lists of (musiq,), the kernel's own value of the returned image
    preds, st1, (sp, s1) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=True, musiq=True, **kw)
    assert all(len(t) == 1 for t in sp + s1)
    _assert_musiq([t[0] for t in sp], preds)
    _assert_musiq([t[0] for t in s1], st1)
    assert [t[0] for t in sp] == [musiq.score_arrays(ctx, p) for p in preds]
    assert len(process(dit, batches[0], 1, "wavelet", False, False, 64, 32, **kw)) == 2
    # with gt=: the value is appended to each tuple, and the rectangle is the ground truth's
    gts = [MM.ramp(192, 200, 1), MM.ramp(31, 256, 2)]
    p2, _, (sg, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, musiq=True, **kw)
    assert all(len(t) == 3 for t in sg) and all(np.array_equal(a, b) for a, b in zip(p2, preds))
    _assert_musiq([t[2] for t in sg], [p[:g.shape[0], :g.shape[1]] for p, g in zip(p2, gts)])
    assert [t[:2] for t in sg] == process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, **kw)[2][0]
    # with niqe= and clipiqa=: (niqe, clipiqa, musiq), the others' values unchanged
    if ctx.__dict__.get("_test_clipiqa_kind") != "small":
        clipiqa.configure(ctx, CM.model("small"))
        ctx.__dict__["_test_clipiqa_kind"] = "small"
    _, _, (sn, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, niqe=NM.params(), clipiqa=True, musiq=True, **kw)
    only = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, niqe=NM.params(), clipiqa=True, **kw)[2][0]
    assert all(len(t) == 3 for t in sn) and [t[:2] for t in sn] == only and [t[2] for t in sn] == [t[0] for t in sp]
    # process_stream(): niqe_rects in step with the batches; the second batch is not scored
    rects = [[(192, 200), (96, 256)], None]
    out = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, musiq=True, niqe_rects=rects, **kw))
    assert [len(r) for r in out] == [3, 2]
    _assert_musiq([t[0] for t in out[0][2][0]], [a[:r[0], :r[1]] for a, r in zip(out[0][0], rects[0])])
    _assert_musiq([t[0] for t in out[0][2][1]], [a[:r[0], :r[1]] for a, r in zip(out[0][1], rects[0])])
    every = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=False, musiq=True, **kw))
    assert [t[0] for t in every[0][2][0]] == [t[0] for t in sp]
    _assert_musiq([t[0] for t in every[1][2][0]], every[1][0])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_musiq_model_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --musiq_model without --gt, --png_encoder gpu --resize gpu: metrics.csv holds `file,musiq` rows that are within the gate of
    the float64 model's score of the DECODED SAVED PNG, and the average line is their mean."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep")
    for i, hw in enumerate([(64, 64), (96, 80)]):
        Image.fromarray((det_input(960 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / ("deep/" if i == 1 else "") / f"im{i}.png")
    MM.EM.save_npz(d / "musiq.npz", MM.model("small"))
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--musiq_model", str(d / "musiq.npz"),
           "--output", str(d / "out"), "--png_encoder", "gpu", "--resize", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = (d / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,musiq"
    got = read_report(str(d / "out" / "metrics.csv"))
    assert sorted(got) == ["deep/im1_0.png", "im0_0.png"]
    gate = MM.gate()[0]
    for k in got:
        want = _model_score(np.array(Image.open(d / "out" / k).convert("RGB")))
        print(f"{k}: musiq {got[k][0]:.12f} (model {want:.12f})")
        assert abs(got[k][0] - want) <= gate, (k, got[k], want)
    assert "were not scored" not in r.stdout and "--musiq_model: scored 2 files" in r.stdout, r.stdout[-1500:]
    assert f"musiq: {np.mean([v[0] for v in got.values()]):.5f}" in r.stdout.splitlines()
