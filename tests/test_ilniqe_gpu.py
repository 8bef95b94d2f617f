"""ir_ilniqe_stats, ir_op_dft2_f64 and ir_op_weibull_fit (csrc/ilniqe.hip) through the C ABI, the pipeline and the command line against the host
model, tools/evaluate_ilniqe.py.

The gates (tests/support/ilniqe_cases.py): plane 0's thirty numbers of every block and the mean / variance of planes 4-6 EQUAL the model's bits
(they pass through no transform, so their floor is 0: the kernel adds, multiplies and takes its logarithm in the model's order); the counts of
every AGGD field equal; the AGGD sums, the Weibull (k, lambda) and the score within 16 times the floor that tests/test_ilniqe_cpu.py measures
between scipy.fft and the dense DFT product inside the model itself (1.08e-16, 5.12e-14, 1.72e-15 relative); no alpha cell may move (the
measured share of cells that move by one step is 0 of 29880, and four times that is 0). The transform is held to 16 times its own floor,
1.46e-15 of the largest output magnitude. The pipeline and command-line tests score images that are no case: their scores are held to
ilniqe_cases.PLUMBING_RTOL, which that file derives."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import ilniqe_cases as IC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EI = IC.EI
CANARY, OUT_CANARY = 0xA5, -777.0
ROW = 2 * 36 * 558


def _ctx():
    from instarevive_amd import ilniqe
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if not ilniqe.configured(ctx):
        ilniqe.configure(ctx)
    return ctx


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- ir_op_dft2_f64
def _dft(re, im, inverse):
    """ir_op_dft2_f64 with exactly the reported workspace, NaN-prefilled outputs with canaries behind them and behind the workspace."""
    ctx = _ctx()
    n = re.shape[0]
    need = ctx.ws_bytes(L.STAGE_ILNIQE_DFT, 1, n, n)
    assert need == 2 * n * n * 8
    d_re = torch.from_numpy(np.ascontiguousarray(re, np.float64)).cuda()
    d_im = None if im is None else torch.from_numpy(np.ascontiguousarray(im, np.float64)).cuda()
    outs = [torch.full((n * n + 4,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    for o in outs:
        o[n * n:] = OUT_CANARY
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_op_dft2_f64(ctx.h, ctx.stream(), L.ptr(d_re), L.ptr(d_im), n, int(inverse), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(ws), need), "ir_op_dft2_f64")
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    assert all(np.all(r[n * n:] == OUT_CANARY) for r in res), "values behind an output were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    assert not any(np.isnan(r).any() for r in res), "an output value was not written"
    return res[0][:n * n].reshape(n, n), res[1][:n * n].reshape(n, n)


@pytest.mark.parametrize("n", [252, 504])
def test_dft_impulses_are_exact(n):
    c, s = EI.twiddles(n)
    x = np.zeros((n, n))
    x[0, 0] = 1.0
    for im in (None, np.zeros((n, n))):
        re, imag = _dft(x, im, False)
        assert np.array_equal(re, np.ones((n, n))) and np.array_equal(imag, np.zeros((n, n)))
    re, imag = _dft(x, None, True)
    assert np.array_equal(re, np.full((n, n), 1.0 / (float(n) * n))) and np.array_equal(imag, np.zeros((n, n)))
    x = np.zeros((n, n))
    x[1, 0] = 1.0                                  # out[j][k] = exp(-2 pi i j / n): the twiddle column, for every k
    re, imag = _dft(x, None, False)
    assert np.array_equal(re, np.repeat(c[:, 1:2], n, 1)) and np.array_equal(imag, np.repeat(-s[:, 1:2], n, 1))
    x = np.zeros((n, n))
    x[0, 1] = 1.0                                  # the twiddle row; through the imaginary input it turns by i
    re, imag = _dft(x, None, False)
    assert np.array_equal(re, np.repeat(c[1:2], n, 0)) and np.array_equal(imag, np.repeat(-s[1:2], n, 0))
    re, imag = _dft(np.zeros((n, n)), x, True)
    inv = 1.0 / (float(n) * n)
    assert np.array_equal(re, np.repeat(-s[1:2], n, 0) * inv) and np.array_equal(imag, np.repeat(c[1:2], n, 0) * inv)


@pytest.mark.parametrize("n", [252, 504])
def test_dft_cosine_seeded_input_and_round_trip(n):
    tol = IC.FACTOR * IC.DFT_FLOOR
    c, _ = EI.twiddles(n)
    r, k = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    re, imag = _dft(c[1][(3 * r + 5 * k) % n], None, False)            # cos(2 pi (3 r + 5 c) / n): bins (3, 5) and (n - 3, n - 5)
    want = np.zeros((n, n))
    want[3, 5] = want[n - 3, n - 5] = n * n / 2.0
    assert np.abs(re - want).max() <= tol * n * n / 2.0 and np.abs(imag).max() <= tol * n * n / 2.0
    x_re, x_im = IC.dft_input(n)
    for inverse in (False, True):
        for im in (x_im, None):
            got = _dft(x_re, im, inverse)
            ref = EI.dft2_scipy(x_re, im, inverse)
            scale = np.abs(ref[0] + 1j * ref[1]).max()
            dev = max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()) / scale
            edge = max(np.abs(g - f)[n - 8:].max() for g, f in zip(got, ref)), max(np.abs(g - f)[:, n - 8:].max() for g, f in zip(got, ref))
            print(f"{n} {'inverse' if inverse else 'forward'} {'complex' if im is not None else 'real'}: {dev:.3e} of the largest magnitude (tolerance {tol:.3e})")
            assert dev <= tol
            assert max(edge) <= tol * scale and all(np.abs(g[n - 8:]).max() > 0 and np.abs(g[:, n - 8:]).max() > 0 for g in got)   # the padded last tile
    fwd = _dft(x_re, x_im, False)
    back = _dft(fwd[0], fwd[1], True)
    # the inverse (scaled by 1 / n^2) passes an error of its input on at most unamplified, and adds its own
    bound = tol * (np.abs(fwd[0] + 1j * fwd[1]).max() + np.abs(x_re + 1j * x_im).max())
    assert max(np.abs(back[0] - x_re).max(), np.abs(back[1] - x_im).max()) <= bound
    again = _dft(x_re, x_im, False)
    assert np.array_equal(_bits(again[0]), _bits(fwd[0])) and np.array_equal(_bits(again[1]), _bits(fwd[1]))


def test_dft_and_weibull_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    n = 252
    x = torch.zeros((n * n,), dtype=torch.float64, device="cuda")
    outs = [torch.full((n * n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    need = ctx.ws_bytes(L.STAGE_ILNIQE_DFT, 1, n, n)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(size=n, re=L.ptr(x), o0=L.ptr(outs[0]), o1=L.ptr(outs[1]), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_op_dft2_f64(handle, ctx.stream(), re, None, size, 0, o0, o1, pw, wsb)

    assert call(size=256) == -1 and call(size=0) == -1 and call(size=503) == -1
    assert call(re=None) == -1 and call(o0=None) == -1 and call(o1=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    assert call(wsb=need - 1) == -1 and call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1 and call(o1=C.c_void_p(outs[1].data_ptr() + 4)) == -1
    assert b"ir_op_dft2_f64" in ctx.lib.ir_last_error(ctx.h)
    k_l = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    wb = lambda rows=2, count=100, px=L.ptr(x), po=L.ptr(k_l), handle=ctx.h: ctx.lib.ir_op_weibull_fit(handle, ctx.stream(), px, rows, count, po)
    assert wb(rows=0) == -1 and wb(count=1) == -1 and wb(count=7057) == -1 and wb(px=None) == -1 and wb(po=None) == -1 and wb(handle=None) == -1
    assert wb(po=C.c_void_p(k_l.data_ptr() + 4)) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + [k_l]) and bool((ws == CANARY).all())
    assert call() == 0


def test_calls_before_configure_are_refused():
    """A context without the bound tables refuses both calls that need them and writes nothing."""
    from instarevive_amd import ilniqe
    ctx = L.Context(0)
    n = 252
    x = torch.zeros((n * n,), dtype=torch.float64, device="cuda")
    outs = [torch.full((n * n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2)]
    ws = torch.empty((ctx.ws_bytes(L.STAGE_ILNIQE, 1, 24, 24),), dtype=torch.uint8, device="cuda")
    assert ctx.lib.ir_op_dft2_f64(ctx.h, ctx.stream(), L.ptr(x), None, n, 0, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(ws), ws.numel()) == -1
    assert b"ir_ilniqe_configure" in ctx.lib.ir_last_error(ctx.h)
    img = torch.from_numpy(IC.cases()["up_24x24"]).cuda()
    plan = torch.from_numpy(ilniqe.plan_host(24, 24).copy()).cuda()
    out = torch.full((ROW,), float("nan"), dtype=torch.float64, device="cuda")
    assert ctx.lib.ir_ilniqe_stats(ctx.h, ctx.stream(), L.ptr(img), 24, 72, 1, 24, 24, L.ptr(plan), L.ptr(out), L.ptr(ws), ws.numel()) == -1
    assert ctx.lib.ir_ilniqe_configure(ctx.h) == -2 and b"ilniqe.win5" in ctx.lib.ir_last_error(ctx.h)      # nothing uploaded yet
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs + [out])


# ---------------------------------------------------------------------------------------------------------------- ir_op_weibull_fit
@pytest.mark.parametrize("rows", [1, 27, 64])
def test_weibull_fit_equals_the_model(rows):
    from instarevive_amd import ilniqe
    named = IC.weibull_rows()
    names = [list(named)[i % len(named)] for i in range(rows)] if rows > 1 else ["many_steps_b"]
    x = np.stack([named[k] for k in names])
    k, lam = ilniqe.weibull_fit(_ctx(), x)
    mk, ml = EI.weibull_fit(x)
    tol = IC.tolerance("weibull")
    for i, name in enumerate(names):
        if np.isnan(mk[i]):
            assert np.isnan(k[i]) and np.isnan(lam[i]), name
            continue
        print(f"{name}: k {k[i]:.15g} (model {mk[i]:.15g}), lambda {lam[i]:.15g} (model {ml[i]:.15g})")
        assert abs(k[i] - mk[i]) <= tol * abs(mk[i]) and abs(lam[i] - ml[i]) <= tol * abs(ml[i]), name
    full = np.abs(np.random.default_rng(3).standard_normal((2, 7056))) + 1e-3       # a whole scale-1 block: the LDS row at its full length
    k, lam = ilniqe.weibull_fit(_ctx(), full)
    mk, ml = EI.weibull_fit(full)
    assert np.abs(k / mk - 1).max() <= tol and np.abs(lam / ml - 1).max() <= tol


# ---------------------------------------------------------------------------------------------------------------- ir_ilniqe_stats
def _call(buf: np.ndarray, h: int, w: int):
    """ir_ilniqe_stats on buf [n][rows][pitch] (bytes) with exactly the reported workspace -> [n][2][36][558]. `out` is NaN-prefilled with four
    canary values behind it and the workspace has 16 canary bytes behind its stated size."""
    from instarevive_amd import ilniqe
    ctx = _ctx()
    n, rows, pitch = buf.shape
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    out = torch.full((n * ROW + 4,), float("nan"), dtype=torch.float64, device="cuda")
    out[n * ROW:] = OUT_CANARY
    need = ctx.ws_bytes(L.STAGE_ILNIQE, n, h, w)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_ilniqe_stats(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(ilniqe.plan(ctx, h, w)), L.ptr(out), L.ptr(ws), need), "ir_ilniqe_stats")
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[n * ROW:] == OUT_CANARY), "values behind out were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return res[:n * ROW].reshape(n, 2, 36, 558).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


@pytest.fixture(scope="module")
def device_stats():
    """{case: [2][36][558]} of every input, one call each; computed once."""
    return {name: _call(_tight([img]), img.shape[0], img.shape[1])[0] for name, img in IC.cases().items()}


@pytest.mark.parametrize("name", list(IC.SIZES))
def test_statistics_alphas_and_score_against_the_model(name, device_stats):
    from instarevive_amd import ilniqe
    dev = device_stats[name]
    stats, feat, score = IC.model(name)
    assert not np.isnan(dev).any()
    assert np.array_equal(_bits(dev[:, :, :30]), _bits(stats[:, :, :30])), "plane 0's thirty numbers"
    assert IC.counts_equal(dev, stats)
    devs = {k: IC.kind_deviation(dev, stats, k) for k in IC.KINDS}
    one, more, total = IC.alpha_cells(dev, stats)
    got = ilniqe.score(ilniqe.features_from_stats(dev), IC.params())
    print(f"{name}: " + ", ".join(f"{k} {v:.3e} (tolerance {IC.tolerance(k):.3e})" for k, v in devs.items())
          + f"; alpha cells off by one {one}, by more {more} of {total}; score {got:.15g} (model {score:.15g}, {abs(got - score) / score:.3e}, tolerance {IC.tolerance('score'):.3e})")
    for k, v in devs.items():
        assert v <= IC.tolerance(k), k
    assert more == 0 and one <= IC.ALPHA_FACTOR * IC.ALPHA_SHARE * total
    assert abs(got - score) <= IC.tolerance("score") * score


def test_flat_quarter_returns_and_plane_0_equals_the_model():
    from instarevive_amd import ilniqe
    img = IC.flat_case()
    dev = _call(_tight([img]), img.shape[0], img.shape[1])[0]
    stats, feat, _ = IC.model(IC.FLAT)
    assert np.array_equal(_bits(dev[:, :, :30]), _bits(stats[:, :, :30]))
    got = ilniqe.features_from_stats(dev)
    cols = np.concatenate([np.arange(18), 234 + np.arange(18)])                   # plane 0's features of both scales
    assert np.isnan(feat[:, cols]).any() and np.array_equal(np.isnan(got[:, cols]), np.isnan(feat[:, cols]))


def test_rectangle_addressing_batch_and_second_call(device_stats):
    """Nothing outside h x w counts: an image embedded with rows > h and a wide pitch gives the bits of the plain one; a batch gives each image its
    own bits, and a second call the same."""
    name = "mixed_40x700"
    img = IC.cases()[name]
    h, w = img.shape[:2]
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 256, (1, h + 9, 3 * w + 37), dtype=np.uint8)
    buf[0, :h, :3 * w] = img.reshape(h, 3 * w)
    assert np.array_equal(_bits(_call(buf, h, w)[0]), _bits(device_stats[name]))
    other = IC.make(h, w, 7200)
    batch = _call(_tight([img, other, img]), h, w)
    assert np.array_equal(_bits(batch[0]), _bits(device_stats[name])) and np.array_equal(_bits(batch[2]), _bits(device_stats[name]))
    assert np.array_equal(_bits(batch[1]), _bits(_call(_tight([other]), h, w)[0])) and not np.array_equal(_bits(batch[1]), _bits(batch[0]))
    assert np.array_equal(_bits(_call(_tight([img, other, img]), h, w)), _bits(batch))


def test_stats_bad_arguments_are_refused_and_write_nothing(device_stats):
    from instarevive_amd import ilniqe
    ctx = _ctx()
    img_np = IC.cases()["up_24x24"]
    h, w = 24, 24
    img = torch.from_numpy(img_np).cuda()
    out = torch.full((ROW + 4,), float("nan"), dtype=torch.float64, device="cuda")
    need = ctx.ws_bytes(L.STAGE_ILNIQE, 1, h, w)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    plan = ilniqe.plan(ctx, h, w)

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(img), pp=L.ptr(plan), po=L.ptr(out), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_ilniqe_stats(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, pp, po, pw, wsb)

    assert call(n=0) == -1 and call(hh=1) == -1 and call(ww=1) == -1
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    assert call(wsb=need - 1) == -1 and call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1
    assert call(pi=None) == -1 and call(pp=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((ws == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[:ROW].cpu().numpy().reshape(2, 36, 558)), _bits(device_stats["up_24x24"]))


def test_score_arrays_is_the_models_score():
    from instarevive_amd import ilniqe
    score = IC.model("down_600x1100")[2]
    assert abs(ilniqe.score_arrays(_ctx(), IC.cases()["down_600x1100"], IC.params()) - score) <= IC.tolerance("score") * score
    with pytest.raises(ilniqe.IlniqeError):
        ilniqe.score_arrays(_ctx(), np.zeros((1, 50, 3), np.uint8), IC.params())


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _assert_ilniqe(values, arrays):
    assert len(values) == len(arrays)
    for v, arr in zip(values, arrays):
        want = IC.model_score(arr)
        print(f"{arr.shape[0]} x {arr.shape[1]}: ilniqe {v:.12f} (model {want:.12f})")
        assert (np.isnan(v) and np.isnan(want)) or abs(v - want) <= IC.PLUMBING_RTOL * want, (v, want)


def test_process_and_process_stream_score_the_returned_images():
    """process(ilniqe=) and process_stream(ilniqe=) on the reduced models, alone, with gt= and with niqe=: the extra element holds the model's
    score of the image the same call returns, right behind NIQE's value."""
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support import niqe_model as NM
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    _ctx()
    params = IC.params()
    batches = [[(det_input(800 + 2 * b + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    preds, st1, (sp, s1) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=True, ilniqe=params, **kw)
    assert all(len(t) == 1 for t in sp + s1)
    _assert_ilniqe([t[0] for t in sp], preds)
    _assert_ilniqe([t[0] for t in s1[:1]], st1[:1])
    assert len(process(dit, batches[0], 1, "wavelet", False, False, 64, 32, **kw)) == 2
    # with gt= and niqe=: (psnr_y, ssim_y, niqe, ilniqe), on the ground truth's rectangle
    gts = [NM.ramp(192, 200, 1), NM.ramp(100, 256, 2)]
    p2, _, (sg, _) = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, niqe=NM.params(), ilniqe=params, **kw)
    assert all(len(t) == 4 for t in sg) and all(np.array_equal(a, b) for a, b in zip(p2, preds))
    _assert_ilniqe([t[3] for t in sg], [p[:g.shape[0], :g.shape[1]] for p, g in zip(p2, gts)])
    three = process(dit, batches[0], 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, niqe=NM.params(), **kw)[2][0]
    assert [t[:3] for t in sg] == three
    # process_stream(): niqe_rects in step with the batches; the first batch is not scored
    rects = [None, [(192, 200), (96, 256)]]
    out = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=False, ilniqe=params, niqe_rects=rects, **kw))
    assert [len(r) for r in out] == [2, 3]
    _assert_ilniqe([t[0] for t in out[1][2][0]], [a[:r[0], :r[1]] for a, r in zip(out[1][0], rects[1])])


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_ilniqe_params_writes_the_models_scores_of_the_saved_files(tmp_path):
    """inference.py --ilniqe_params without --gt, --png_encoder gpu --resize gpu, on three small files: metrics.csv holds `file,ilniqe` rows that
    equal the model's score of the DECODED SAVED PNG; with --niqe_params as well both columns appear."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.support import niqe_model as NM
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep")
    for i, hw in enumerate([(192, 192), (192, 256), (64, 64)]):
        Image.fromarray((det_input(950 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / ("deep/" if i == 1 else "") / f"im{i}.png")
    IC.write_mat(d / "ILNIQE_templateModel.mat")
    mu, cov = NM.params()
    np.savez(d / "pristine.npz", mu_prisparam=mu, cov_prisparam=cov)
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
            str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
            "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--ilniqe_params", str(d / "ILNIQE_templateModel.mat"),
            "--png_encoder", "gpu", "--resize", "gpu"]
    r = subprocess.run(base + ["--output", str(d / "out")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (d / "out" / "metrics.csv").read_text().splitlines()[0] == "file,ilniqe"
    names = sorted(os.path.relpath(os.path.join(dp, f), d / "out") for dp, _, fs in os.walk(d / "out") for f in fs if f.endswith(".png"))
    assert len(names) == 3
    want = {k: IC.model_score(np.array(Image.open(d / "out" / k).convert("RGB"))) for k in names}
    got = read_report(str(d / "out" / "metrics.csv"))
    assert sorted(got) == names and not any(np.isnan(v) for v in want.values())
    for k, v in want.items():
        assert abs(got[k][0] - v) <= IC.PLUMBING_RTOL * v, (k, got[k], v)
    assert f"ilniqe: {np.mean(list(want.values())):.5f}" in r.stdout.splitlines()
    r = subprocess.run(base + ["--output", str(d / "both"), "--niqe_params", str(d / "pristine.npz")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (d / "both" / "metrics.csv").read_text().splitlines()[0] == "file,niqe,ilniqe"
    both = read_report(str(d / "both" / "metrics.csv"))
    assert both and set(both) <= set(names) and all(v[1] == got[k][0] for k, v in both.items())   # the same image gives the same bits; NIQE leaves the 64 x 64 file out
