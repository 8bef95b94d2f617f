"""ir_niqe_stats (csrc/niqe.hip) through the C ABI, the pipeline and the command line against the host model, tools/evaluate_niqe.py.

The gates (tests/support/niqe_model.py): the twenty counts of every block EQUAL the model's - on the flat patches and the grey ramp y - mu is
rounding noise, so this holds only when the kernel adds in the model's order; the sums within 1e-10 relative (reordering 9216 fp64 terms is
bounded by 9216 * 2^-53 ~ 1e-12, x100 for the divide and the square root); the alphas fitted from the device's statistics equal; the score within
1e-9 relative. tests/test_niqe_cpu.py shows that every input keeps its rn 1e-9 away from the points where alpha flips, and that a separable or
reordered filter misses these gates."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import niqe_model as NM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _call(buf: np.ndarray, h: int, w: int):
    """ir_niqe_stats on buf [n][rows][pitch] (bytes) with exactly the reported workspace -> [n][2][blocks][5][6]. `out` has four canary values
    behind it and the workspace 16 canary bytes behind its stated size: both must stay untouched."""
    ctx = _ctx()
    n, rows, pitch = buf.shape
    nb = (h // 96) * (w // 96)
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    out = torch.full((n * nb * 60 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_NIQE, n, h, w)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_niqe_stats(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(out), L.ptr(ws), need), "ir_niqe_stats")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[n * nb * 60:] == OUT_CANARY), "values behind out were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return res[:n * nb * 60].reshape(n, 2, nb, 5, 6).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def device_stats():
    """{case: [2][blocks][5][6]} of every input, one call each; computed once."""
    return {name: _call(_tight([img]), img.shape[0], img.shape[1])[0] for name, img in NM.cases().items()}


@pytest.mark.parametrize("name", list(NM.cases()))
def test_statistics_alphas_and_score_equal_the_model(name, device_stats):
    from instarevive_amd import niqe
    dev = device_stats[name]
    stats, feat, score = NM.model(name)
    assert dev.shape == stats.shape
    counts, dev_sums = NM.compare_stats(dev, stats)
    print(f"{name}: counts equal {counts}, largest relative deviation of the sums {dev_sums:.3e}")
    assert counts, np.argwhere(dev[..., :2] != stats[..., :2])[:8]
    assert dev_sums <= NM.SUM_RTOL
    got = niqe.features_from_stats(dev)
    assert np.array_equal(NM.alphas(got), NM.alphas(feat))
    assert np.array_equal(np.isnan(got), np.isnan(feat))
    if score is None:
        with pytest.raises(niqe.NiqeError):
            niqe.score(got, NM.params())
    else:
        mine = niqe.score(got, NM.params())
        print(f"{name}: niqe {mine:.12f} (model {score:.12f}), relative {abs(mine - score) / score:.3e}")
        assert abs(mine - score) <= NM.SCORE_RTOL * score


def test_nothing_outside_the_scored_rectangle_counts(device_stats):
    """200 x 300 scored twice with different garbage outside 192 x 288: bit-equal, and equal to the 192 x 288 image alone."""
    a, b, alone = (device_stats[k] for k in ("patches_in_200x300_a", "patches_in_200x300_b", "patches_192x288"))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(alone))


def test_embedded_image_with_rows_and_pitch(device_stats):
    """rows > h and pitch > 3 w: the same bits as the tight image."""
    img = NM.cases()["noise_192x288"]
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1, 201, 3 * 288 + 37), dtype=np.uint8)
    buf[0, :192, :3 * 288] = img.reshape(192, -1)
    assert np.array_equal(_bits(_call(buf, 192, 288)[0]), _bits(device_stats["noise_192x288"]))


def test_a_batch_gives_each_image_its_own_bits_and_a_second_call_the_same(device_stats):
    names = ["noise_192x288", "patches_192x288", "noise_192x288"]
    imgs = [NM.cases()[k] for k in names]
    batch = _call(_tight(imgs), 192, 288)
    for got, k in zip(batch, names):
        assert np.array_equal(_bits(got), _bits(device_stats[k])), k
    assert np.array_equal(_bits(_call(_tight(imgs), 192, 288)), _bits(batch))


def test_bad_arguments_are_refused_and_write_nothing(device_stats):
    ctx = _ctx()
    h, w = 96, 192
    img = torch.from_numpy(NM.cases()["ramp_96x192"]).cuda()
    out = torch.full((2 * 60 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_NIQE, 1, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(img), po=L.ptr(out), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_niqe_stats(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, po, pw, wsb)

    assert call(n=0) == -1 and call(hh=95) == -1 and call(ww=95) == -1
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(pi=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[:120].cpu().numpy().reshape(2, 2, 5, 6)), _bits(device_stats["ramp_96x192"]))


def test_score_arrays_is_the_models_score():
    from instarevive_amd import niqe
    img = NM.cases()["zero_block_480x672"]
    score = NM.model("zero_block_480x672")[2]
    assert abs(niqe.score_arrays(_ctx(), img, NM.params()) - score) <= NM.SCORE_RTOL * score
    with pytest.raises(niqe.NiqeError):
        niqe.score_arrays(_ctx(), NM.cases()["noise_96x96"], NM.params())      # one block: one feature row
    with pytest.raises(niqe.NiqeError):
        niqe.score_arrays(_ctx(), NM.noise(95, 200, 1), NM.params())


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _model_score(arr):
    """The model's score of an array, NaN where it has none."""
    if min(arr.shape[:2]) < 96:
        return float("nan")
    try:
        return NM.EN.niqe(arr, *NM.params())
    except ValueError:
        return float("nan")


def _assert_niqe(values, arrays):
    assert len(values) == len(arrays)
    for v, arr in zip(values, arrays):
        want = _model_score(arr)
        print(f"{arr.shape[0]} x {arr.shape[1]}: niqe {v:.12f} (model {want:.12f})")
        assert (np.isnan(v) and np.isnan(want)) or abs(v - want) <= NM.SCORE_RTOL * want, (v, want)


def test_process_and_process_stream_score_the_returned_images():
    """process(niqe=) and process_stream(niqe=) on the reduced models, with and without gt=: the extra element holds the model's score of the
    image the same call returns - the whole output, a rectangle given by niqe_rects or by the ground truth's size - for predictions and stage-1
    images; a batch whose niqe_rects entry is None is not scored."""
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    params = NM.params()
    batches = [[(det_input(800 + 2 * b + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(3)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    # process(), alone: a pair of lists of (niqe,)
    preds, st1, (sp, s1) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=True, niqe=params, **kw)
    assert all(len(t) == 1 for t in sp + s1)
    _assert_niqe([t[0] for t in sp], preds)
    _assert_niqe([t[0] for t in s1], st1)
    assert len(process(dit, batches[0], 1, "wavelet", False, False, 64, 32, **kw)) == 2
    # with gt=: the value is appended to each tuple, and the rectangle is the ground truth's
    gts = [NM.ramp(192, 200, 1), NM.ramp(100, 256, 2)]
    p2, _, (sg, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, niqe=params, **kw)
    assert all(len(t) == 3 for t in sg) and all(np.array_equal(a, b) for a, b in zip(p2, preds))
    _assert_niqe([t[2] for t in sg], [p[:g.shape[0], :g.shape[1]] for p, g in zip(p2, gts)])
    paired = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, **kw)[2][0]
    assert [t[:2] for t in sg] == paired
    # process_stream(): niqe_rects in step with the batches; the middle batch is not scored
    rects = [[(192, 256), (192, 256)], None, [(192, 200), (96, 256)]]
    out = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, niqe=params, niqe_rects=rects, **kw))
    assert [len(r) for r in out] == [3, 2, 3]
    for b in (0, 2):
        _assert_niqe([t[0] for t in out[b][2][0]], [a[:r[0], :r[1]] for a, r in zip(out[b][0], rects[b])])
        _assert_niqe([t[0] for t in out[b][2][1]], [a[:r[0], :r[1]] for a, r in zip(out[b][1], rects[b])])
    # without niqe_rects every batch is scored on the whole output; with gt= the batches that have ground truth
    every = list(process_stream(dit, batches[:2], "wavelet", False, False, 64, 32, return_stage1=False, niqe=params, **kw))
    for r in every:
        _assert_niqe([t[0] for t in r[2][0]], r[0])
    both = list(process_stream(dit, batches[:2], "wavelet", False, False, 64, 32, return_stage1=False, niqe=params, gt=[gts, None], **kw))
    assert [len(r) for r in both] == [3, 2] and all(len(t) == 3 for t in both[0][2][0])
    _assert_niqe([t[2] for t in both[0][2][0]], [p[:g.shape[0], :g.shape[1]] for p, g in zip(both[0][0], gts)])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_niqe_params_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --niqe_params without --gt, --png_encoder gpu --resize gpu: metrics.csv holds `file,niqe` rows that equal the model's score of the
    DECODED SAVED PNG; the file below 96 pixels is counted, not scored."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep")
    for i, hw in enumerate([(512, 512), (512, 576), (64, 64)]):
        Image.fromarray((det_input(950 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / ("deep/" if i == 1 else "") / f"im{i}.png")
    mu, cov = NM.params()
    np.savez(d / "pristine.npz", mu_prisparam=mu, cov_prisparam=cov)
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--niqe_params", str(d / "pristine.npz"),
           "--output", str(d / "out"), "--png_encoder", "gpu", "--resize", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = (d / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,niqe"
    want = {}
    for k in ("im0_0.png", "deep/im1_0.png"):
        want[k] = _model_score(np.array(Image.open(d / "out" / k).convert("RGB")))
    got = read_report(str(d / "out" / "metrics.csv"))
    scorable = {k: v for k, v in want.items() if not np.isnan(v)}
    assert sorted(got) == sorted(scorable)
    for k, v in scorable.items():
        assert abs(got[k][0] - v) <= NM.SCORE_RTOL * v, (k, got[k], v)
    assert f"--niqe_params: {3 - len(scorable)} of 3 files were not scored" in r.stdout, r.stdout[-1500:]
    if scorable:
        assert f"niqe: {np.mean(list(scorable.values())):.5f}" in r.stdout.splitlines()
