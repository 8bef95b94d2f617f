"""ir_metrics_y (csrc/metrics.hip) through the C ABI, the pipeline and the command lines against the host model, tools/evaluate_pairs.py.

Tolerance of every comparison with the model: |ssim - model| <= 1e-9 and |mse - model| <= 1e-9 * max(model, 1e-8). The kernel keeps every
statistic in fp64, and fp64 arithmetic in another summation order moves the result by <= 5e-15, while ONE luma value off by one in a 96 x 80 pair
moves SSIM by 1.5e-7: 1e-9 separates the two with two orders of margin on each side (tests/test_metrics_cpu.py shows on the near-tie colours
that a wrong luma rounding misses by > 1e-6). PSNR is 10 log10(1 / (mse + 1e-8)), so the relative bound on the MSE bounds it by 4.4e-9 dB:
the pipeline and command-line tests, which see PSNR, use 1e-8."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import metrics_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
PSNR_TOL = 1e-8


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _call(a_buf: np.ndarray, b_buf: np.ndarray, h: int, w: int):
    """ir_metrics_y on a_buf [n][a_rows][a_pitch] / b_buf [n][b_rows][b_pitch] (bytes) -> [n][2] (mse_y, ssim_y). `out` has four canary values
    behind [n][2] and the workspace 16 canary bytes behind its stated size: both must stay untouched."""
    ctx = _ctx()
    n, a_rows, a_pitch = a_buf.shape
    _, b_rows, b_pitch = b_buf.shape
    da, db = torch.from_numpy(np.ascontiguousarray(a_buf)).cuda(), torch.from_numpy(np.ascontiguousarray(b_buf)).cuda()
    out = torch.full((2 * n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_METRICS, n, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_metrics_y(ctx.h, ctx.stream(), L.ptr(da), a_rows, a_pitch, L.ptr(db), b_rows, b_pitch, n, h, w, L.ptr(out), L.ptr(ws), need), "ir_metrics_y")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[2 * n:] == OUT_CANARY), "values behind out[n][2] were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return res[:2 * n].reshape(n, 2).copy()


def _tight(imgs):
    """[n] HWC images of one size -> [n][h][3 w] bytes."""
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _embed(imgs, rows, pitch, seed):
    """The images in the top-left corner of [n][rows][pitch] buffers whose other bytes are noise."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, (len(imgs), rows, pitch), dtype=np.uint8)
    for i, im in enumerate(imgs):
        buf[i, :im.shape[0], :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    return buf


def _check_against_model(got, pairs):
    for (name, (a, b)), (mse, ssim) in zip(pairs.items(), got):
        ok, (mse, m, ssim, s) = M.within(mse, ssim, a, b)
        print(f"{name} {a.shape[0]} x {a.shape[1]}: mse {mse:.17g} (model {m:.17g}), ssim {ssim:.17g} (model {s:.17g}, off by {abs(ssim - s):.2e})")
        assert ok, (name, mse, m, ssim, s)
        if name == "identical":
            assert mse == 0.0 and ssim == 1.0
        if name == "checker_inverse":
            assert s == 0.0   # the clamp fires on every window


@pytest.mark.parametrize("h,w", [(11, 11), (12, 75), (96, 80), (139, 201)])
def test_every_input_kind_equals_the_model(h, w):
    """One window; one row of windows; more than one tile; remainders in both directions across the 16 x 64 tiles. The eight input kinds of
    one size go through one call as a batch of eight."""
    pairs = M.pairs_for(h, w, seed=h + w)
    got = _call(_tight([p[0] for p in pairs.values()]), _tight([p[1] for p in pairs.values()]), h, w)
    _check_against_model(got, pairs)


def test_rectangle_inside_wider_taller_buffers_of_odd_pitch():
    """520 x 776 of buffers with 577 / 531 rows and pitches of 2501 / 2333 bytes: nothing outside the rectangle may reach the scores."""
    all_pairs = M.pairs_for(520, 776, seed=5)
    pairs = {k: all_pairs[k] for k in ("noise_pm2", "ramp_pm3", "checker_inverse")}
    a = _embed([p[0] for p in pairs.values()], 577, 2501, 1)
    b = _embed([p[1] for p in pairs.values()], 531, 2333, 2)
    _check_against_model(_call(a, b, 520, 776), pairs)


def test_one_1024_pair_equals_the_model():
    r = M.ramp(1024, 1024, 9)
    pairs = {"ramp_pm3": (r, M.shifted(r, 3, 10))}
    _check_against_model(_call(_tight([r]), _tight([pairs["ramp_pm3"][1]]), 1024, 1024), pairs)


def test_near_tie_colours_equal_the_model():
    """The pair of tests/test_metrics_cpu.py::test_near_tie_colours_separate_the_luma_variants: exact-integer or fp32 luma would miss by > 1e-6."""
    a, b = M.near_tie_pair()
    _check_against_model(_call(_tight([a]), _tight([b]), 24, 32), {"near_tie": (a, b)})


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def test_batch_position_and_repetition_do_not_change_a_bit():
    h, w = 139, 201
    ps = [(M.noise(h, w, 1), M.noise(h, w, 2)), (M.ramp(h, w, 3), M.shifted(M.ramp(h, w, 3), 3, 4)), (M.noise(h, w, 5), M.shifted(M.noise(h, w, 5), 2, 6))]
    batch = _call(_tight([p[0] for p in ps]), _tight([p[1] for p in ps]), h, w)
    singles = np.concatenate([_call(_tight([a]), _tight([b]), h, w) for a, b in ps])
    assert np.array_equal(_bits(batch), _bits(singles))
    twice = _call(_tight([ps[0][0], ps[1][0], ps[0][0]]), _tight([ps[0][1], ps[1][1], ps[0][1]]), h, w)
    assert np.array_equal(_bits(twice[0]), _bits(twice[2])) and np.array_equal(_bits(twice[:2]), _bits(batch[:2]))
    again = _call(_tight([p[0] for p in ps]), _tight([p[1] for p in ps]), h, w)
    assert np.array_equal(_bits(again), _bits(batch))


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    h, w = 32, 40
    a = torch.from_numpy(M.noise(h, w, 1)).cuda()
    b = torch.from_numpy(M.noise(h, w, 2)).cuda()
    out = torch.full((6,), OUT_CANARY, dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_METRICS, 1, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pa=L.ptr(a), pb=L.ptr(b), po=L.ptr(out), pw=L.ptr(ws), wsb=need, b_rows=None, b_pitch=None):
        return ctx.lib.ir_metrics_y(ctx.h, ctx.stream(), pa, rows, pitch, pb, rows if b_rows is None else b_rows, pitch if b_pitch is None else b_pitch,
                                    n, hh, ww, po, pw, wsb)

    assert call(n=0) == -1 and call(hh=10) == -1 and call(ww=10) == -1
    assert call(rows=h - 1) == -1 and call(b_rows=h - 1) == -1           # h above a_rows / b_rows
    assert call(pitch=3 * w - 1) == -1 and call(b_pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(pa=None) == -1 and call(pb=None) == -1 and call(po=None) == -1 and call(pw=None) == -1
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    ok, info = M.within(float(out[0]), float(out[1]), a.cpu().numpy(), b.cpu().numpy())
    assert ok, info


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _assert_scores(scores, arrays, gts):
    assert len(scores) == len(arrays) == len(gts)
    for (psnr, ssim), arr, g in zip(scores, arrays, gts):
        arr = arr[:g.shape[0], :g.shape[1]]
        _, p, s = M.model_scores(arr, g)
        print(f"{g.shape[0]} x {g.shape[1]}: psnr {psnr:.12f} (model {p:.12f}), ssim {ssim:.12f} (model {s:.12f})")
        assert abs(psnr - p) <= PSNR_TOL and abs(ssim - s) <= M.SSIM_TOL, (psnr, p, ssim, s)


def _decode(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def test_process_stream_scores_equal_the_model_on_its_own_arrays():
    """process_stream(gt=...) on the reduced models and batches of tests/test_png_gpu.py: the scores of predictions and stage-1 images must be the
    model's on the arrays the same run yields without gt - on rectangles given by the ground truth's own size, on png rectangles (where the
    files are decoded), with a batch that has no ground truth in between, and through process()."""
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    batches = [[(det_input(500 + 2 * b + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(3)]
    rects = [[(64, 128), (64, 128)], [(40, 100), (64, 77)], [(64, 128), (33, 128)]]
    gts = [[M.ramp(vh, vw, 40 + 2 * b + i) for i, (vh, vw) in enumerate(rr)] for b, rr in enumerate(rects)]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    plain = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, **kw))
    scored = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, gt=[gts[0], None, gts[2]], **kw))
    assert [len(r) for r in scored] == [3, 2, 3]
    for b in (0, 1, 2):
        assert all(np.array_equal(x, y_) for x, y_ in zip(plain[b][0] + plain[b][1], scored[b][0] + scored[b][1]))
    for b in (0, 2):
        _assert_scores(scored[b][2][0], plain[b][0], gts[b])
        _assert_scores(scored[b][2][1], plain[b][1], gts[b])
    # graph=True: the scoring runs behind the replay, outside the recording - at most one recording per staging slot (two call signatures) serves
    # the three batches, scored or not
    before = dit.ctx.graph_records
    replayed = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, graph=True, gt=[gts[0], None, gts[2]], **kw))
    assert dit.ctx.graph_records - before <= 2 and [len(r) for r in replayed] == [3, 2, 3]
    for b in (0, 2):
        _assert_scores(replayed[b][2][0], replayed[b][0], gts[b])
        _assert_scores(replayed[b][2][1], replayed[b][1], gts[b])
    # with png= the raw result is not downloaded: decode the files
    coded = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=False, png=rects, gt=gts, **kw))
    for b in range(3):
        preds, st1, (sp, s1) = coded[b]
        assert st1 == [] and s1 == [] and all(isinstance(z, bytes) for z in preds)
        dec = [_decode(z) for z in preds]
        assert all(np.array_equal(d, a[:r[0], :r[1]]) for d, a, r in zip(dec, plain[b][0], rects[b]))
        _assert_scores(sp, dec, gts[b])
    # process() takes the same argument
    preds, st1, (sp, s1) = process(dit, batches[1], 1, "wavelet", False, False, 64, 32, return_stage1=True, gt=gts[1], **kw)
    _assert_scores(sp, plain[1][0], gts[1])
    _assert_scores(s1, plain[1][1], gts[1])
    assert len(process(dit, batches[1], 1, "wavelet", False, False, 64, 32, **kw)) == 2
    # a ground truth of another size is refused with both sizes, before anything is launched for the batch
    wrong = [gts[1][0], M.ramp(64, 78, 1)]
    with pytest.raises(ValueError, match="64 x 78.*64 x 77"):
        list(process_stream(dit, batches[1:2], "wavelet", False, False, 64, 32, png=rects[1:2], gt=[wrong], **kw))
    with pytest.raises(ValueError, match="65 x 128.*64 x 128"):
        process(dit, batches[0], 1, "wavelet", False, False, 64, 32, gt=[gts[0][0], M.ramp(65, 128, 1)], **kw)


def test_process_stream_scores_the_resized_results():
    """process_stream(resize=..., gt=...): one batch whose inputs were enlarged (two) or not (one); the ground truth has the final size - the LANCZOS
    target, else the valid rectangle - and the scores must be the model's on the final arrays of the same run without gt."""
    from instarevive_amd.pipeline import process_stream
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.golden._det import det_input
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    records = [[ResizeJob((det_input(700 + i, (h, w, 3)) * 255).numpy().astype(np.uint8), job_geometry((w, h), 1, True, 64))
                for i, (h, w) in enumerate([(40, 56), (48, 80), (64, 100)])]]
    assert [r.geo.lanczos for r in records[0]] == [(56, 40), (80, 48), None]
    raws = [[r.raw for r in records[0]]]
    gts = [[M.ramp(h, w, 60 + i) for i, (h, w) in enumerate([(40, 56), (48, 80), (64, 100)])]]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    plain = list(process_stream(dit, raws, "wavelet", False, False, 64, 32, return_stage1=True, resize=records, **kw))
    scored = list(process_stream(dit, raws, "wavelet", False, False, 64, 32, return_stage1=True, resize=records, gt=gts, **kw))
    assert len(scored[0]) == 3 and all(np.array_equal(x, y_) for x, y_ in zip(plain[0][0] + plain[0][1], scored[0][0] + scored[0][1]))
    assert [a.shape[:2] for a in plain[0][0]] == [(40, 56), (48, 80), (64, 100)]
    _assert_scores(scored[0][2][0], plain[0][0], gts[0])
    _assert_scores(scored[0][2][1], plain[0][1], gts[0])
    with pytest.raises(ValueError, match="40 x 57.*40 x 56"):
        list(process_stream(dit, raws, "wavelet", False, False, 64, 32, resize=records, gt=[[M.ramp(40, 57, 1)] + gts[0][1:]], **kw))


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _model_rows(out_dir, gt_of):
    """{relative file: model (psnr, ssim) of the decoded saved PNG against gt_of(relative file)}."""
    rows = {}
    for root, _, names in os.walk(out_dir):
        for nm in names:
            if nm.endswith(".png"):
                k = os.path.relpath(os.path.join(root, nm), out_dir)
                rows[k] = M.model_scores(np.array(Image.open(os.path.join(root, nm)).convert("RGB")), gt_of(k))[1:]
    return rows


def _assert_report(path, want):
    from instarevive_amd.metrics import read_report
    got = read_report(str(path))
    assert sorted(got) == sorted(want)
    for k in want:
        assert abs(got[k][0] - want[k][0]) <= PSNR_TOL and abs(got[k][1] - want[k][1]) <= M.SSIM_TOL, (k, got[k], want[k])


def _cli_folder(d):
    """The 17-file folder of five sizes of tests/test_png_gpu.py, a ground-truth tree that mirrors it, and the command line over both."""
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _five_size_folder
    _write_artifacts(d)
    truth = {}
    for i, hw in enumerate(_five_size_folder(d)):   # the saved file of im07.png is im07_0.png
        sub = ("", "deep/", "deep/er/")[i % 3]
        os.makedirs(d / "gt" / sub, exist_ok=True)
        truth[f"{sub}im{i:02d}_0.png"] = M.ramp(hw[0], hw[1], 900 + i)
        Image.fromarray(truth[f"{sub}im{i:02d}_0.png"]).save(d / "gt" / f"{sub}im{i:02d}.png")
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "3", "--workers", "4", "--gt", str(d / "gt")]
    return truth, cmd


def test_cli_gt_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --gt --png_encoder gpu --resize gpu: every file is scored, and metrics.csv holds the model's scores of the decoded saved PNGs."""
    d = tmp_path
    truth, cmd = _cli_folder(d)
    stdout = _run(cmd + ["--output", str(d / "out"), "--png_encoder", "gpu", "--resize", "gpu"])
    assert "were not scored" not in stdout and "--gt: scored 17 files" in stdout, stdout[-1500:]
    want = _model_rows(d / "out", lambda k: truth[k])
    assert len(want) == 17
    _assert_report(d / "out" / "metrics.csv", want)
    avg = [ln for ln in stdout.splitlines() if ln.startswith(("psnr: ", "ssim: "))]
    assert avg == [f"psnr: {np.mean([v[0] for v in want.values()]):.5f}", f"ssim: {np.mean([v[1] for v in want.values()]):.5f}"]


def test_cli_gt_counts_the_files_the_host_resized(tmp_path):
    """Without --resize gpu the fourteen enlarged inputs are saved from an image the host made: they are counted, not scored; the three plain crops
    are scored, into the file --metrics_out names."""
    d = tmp_path
    truth, cmd = _cli_folder(d)
    stdout = _run(cmd + ["--output", str(d / "out"), "--metrics_out", str(d / "host.csv")])
    note = [ln for ln in stdout.splitlines() if "were not scored" in ln]
    assert len(note) == 1 and "--gt: 14 of 17 files were not scored" in note[0] and "use --resize gpu" in note[0], stdout[-1500:]
    want = {k: v for k, v in _model_rows(d / "out", lambda k: truth[k]).items() if min(truth[k].shape[:2]) >= 512}
    assert len(want) == 3
    _assert_report(d / "host.csv", want)


def test_eval_batch_gt_writes_both_reports(tmp_path):
    from instarevive_amd.utils import center_crop_arr
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "lq" / "sub", exist_ok=True)
    os.makedirs(d / "gt" / "sub", exist_ok=True)
    srcs = {"a.png": (70, 90), "b.jpg": (64, 64), "sub/c.png": (150, 130), "d.png": (64, 100), "e.png": (97, 71)}
    truth = {}
    for i, (k, hw) in enumerate(srcs.items()):
        Image.fromarray((det_input(80 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "lq" / k, quality=95)
        stem = os.path.splitext(k)[0]
        Image.fromarray(M.ramp(hw[0] + 9, hw[1] + 5, 30 + i)).save(d / "gt" / (stem + ".png"))   # another size: centre-cropped like the input
        truth[stem + ".png"] = np.ascontiguousarray(center_crop_arr(Image.open(d / "gt" / (stem + ".png")).convert("RGB"), 64))
    stdout = _run([sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "lq"), "--output",
                   str(d / "res"), "--cond_output", str(d / "cond"), "--batch_size", "2", "--image_size", "64", "--swinir_ckpt",
                   str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
                   "--prompt_embeds", str(d / "prompt.pth"), "--gt", str(d / "gt")])
    for folder in ("res", "cond"):
        want = _model_rows(d / folder, lambda k: truth[k])
        assert len(want) == len(srcs)
        _assert_report(d / folder / "metrics.csv", want)
    assert len([ln for ln in stdout.splitlines() if ln.startswith("psnr: ")]) == 2 and len([ln for ln in stdout.splitlines() if ln.startswith("ssim: ")]) == 2


def test_evaluate_pairs_gpu_backend_prints_the_host_lines(tmp_path):
    for i, (h, w) in enumerate([(64, 64), (40, 90), (139, 201)]):
        os.makedirs(tmp_path / "a", exist_ok=True)
        os.makedirs(tmp_path / "b", exist_ok=True)
        r = M.ramp(h, w, 70 + i)
        Image.fromarray(r).save(tmp_path / "a" / f"im{i}.png")
        Image.fromarray(M.shifted(r, 3, 80 + i)).save(tmp_path / "b" / f"im{i}.png")
    host = []
    M.EP.evaluate(str(tmp_path / "a"), str(tmp_path / "b"), log=host.append)
    stdout = _run([sys.executable, os.path.join(ROOT, "tools", "evaluate_pairs.py"), "-i", str(tmp_path / "a"), "-r", str(tmp_path / "b"), "--backend", "gpu"])
    lines = [ln for ln in stdout.splitlines() if ln.startswith(("Find ", "psnr: ", "ssim: "))]
    assert lines == host and len(host) == 3
