"""ir_degrade_chain (csrc/degrade_chain.hip) through the C ABI, the pipeline and the command line against the numpy model,
tools/degrade_folder.py:degrade_chain_model.

The gate is equality: of the LQ bytes, and bit for bit of the float32 image behind the op under test (`tap`), with no tolerance - every op is
a fixed sequence of IEEE operations that the model performs in the same order, on tables (exp, the DCT basis) that numpy computed for both."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from instarevive_amd import _lib as L
from instarevive_amd import degrade as D
from tools import degrade_folder as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
QUALITIES = (30.5, 49.9, 95.0)
F, R, G, P, J = L.CHAIN_FILTER, L.CHAIN_RESIZE, L.CHAIN_GAUSS, L.CHAIN_POISSON, L.CHAIN_DIFFJPEG
AREA, LIN, CUB = L.CHAIN_AREA, L.CHAIN_BILINEAR, L.CHAIN_BICUBIC


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _image(h, w, seed=0):
    rng = np.random.default_rng([h, w, seed])
    walk = np.cumsum(np.cumsum(rng.normal(0, 1.5, (h, w, 3)), 0), 1) * 0.3
    img = np.clip(128 + walk, 0, 255).astype(np.uint8)
    img[: h // 3] = rng.integers(0, 256, (h // 3, w, 3), dtype=np.uint8)   # texture: every DCT coefficient busy
    return img


def _kernel(K=21):
    return D.pad_kernel(D.generalized_gaussian(min(K, 13), 2.5, 0.9, -1.1, 1.7, False), K)


def _normal(shape, seed=1):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def _uniform(shape, seed=2):
    return np.random.default_rng(seed).random(shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(img, ops, taps):
    """One device call with the image once per tap; bytes and every tapped float image against the model."""
    p = D.ChainParams(tuple(ops))
    lq, got = D.degrade_chain(_ctx(), [img] * len(taps), [p] * len(taps), taps=list(taps))
    for i, t in enumerate(taps):
        want_lq, want = M.degrade_chain_model(img, ops, tap=t)
        assert got[i].shape == want.shape, (t, got[i].shape, want.shape)
        bad = np.argwhere(_bits(got[i]) != _bits(want))
        assert bad.size == 0, (f"op {t} (kind {ops[t][0]})", len(bad), bad[:4], got[i][tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(lq[i], want_lq), (t, np.argwhere(lq[i] != want_lq)[:4])
    return lq[0]


# ---------------------------------------------------------------- one op at a time
@pytest.mark.parametrize("hw", [(11, 16), (33, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_k21(hw):
    """11 x 16: the reflection reaches the whole image; 33 x 70: patch borders in both directions."""
    lq = _check(_image(*hw), [(F, _kernel(21))], [0])
    assert not np.array_equal(lq, _image(*hw))


def test_filter_smaller_kernels_and_the_delta():
    img = _image(20, 45)
    _check(img, [(F, _kernel(7)), (F, D.circular_lowpass_kernel(1.3, 13))], [0, 1])
    assert np.array_equal(_check(img, [(F, D.delta_kernel(21))], [0]), img)


@pytest.mark.parametrize("mode", [AREA, LIN, CUB], ids=["area", "bilinear", "bicubic"])
def test_resize_down_up_and_by_scale_factor(mode):
    _check(_image(37, 53), [(R, mode, 13, 19, 0.0), (R, CUB, 37, 53, 0.0)], [0, 1])          # down by size=, odd sizes
    _check(_image(13, 19), [(R, mode, 19, 28, 1.5), (R, AREA, 13, 19, 0.0)], [0, 1])         # up by scale_factor=
    _check(_image(37, 53), [(R, mode, 13, 19, 0.37), (R, LIN, 37, 53, 0.0)], [0, 1])         # down by scale_factor=: 1 / 0.37 is not 37 / 13
    _check(_image(37, 53), [(R, mode, 37, 53, 1.0)], [0])                                    # keep


def test_bicubic_times_four():
    _check(_image(12, 16), [(R, CUB, 48, 64, 0.0), (R, LIN, 12, 16, 0.0)], [0, 1])


def _levels_image(kind, h=24, w=32):
    if kind == "one":
        return np.full((h, w, 3), 77, dtype=np.uint8)
    img = np.resize(np.arange(256, dtype=np.uint8), (h, w, 3)).copy()   # 256 distinct levels
    assert len(np.unique(img)) == 256
    return img


@pytest.mark.parametrize("gray", [False, True], ids=["colour", "gray"])
def test_gauss_and_poisson(gray):
    h, w = 24, 32
    shape = (h, w) if gray else (h, w, 3)
    _check(_image(h, w), [(G, _normal(shape), 12.5, gray), (P, _uniform(shape), 1.25, gray), (G, _normal(shape, 3), 30.0, gray)], [0, 1, 2])
    for kind in ("one", "256"):
        img = _levels_image(kind)
        lq = _check(img, [(P, _uniform(shape, 7), 2.5, gray)], [0])
        assert not np.array_equal(lq, img)
    _check(_image(37, 53), [(R, AREA, 17, 23, 0.0), (P, _uniform((17, 23) if gray else (17, 23, 3), 9), 0.05, gray), (R, CUB, 37, 53, 0.0)], [1])


def test_poisson_with_uniforms_at_the_ends():
    """u = 0 (k = 0 at once) and u just below 1 (the loop runs far into the tail): the loop's ends."""
    img = _levels_image("256")
    u = _uniform(img.shape, 11)
    u[0, :8] = 0.0
    u[1, :8] = np.nextafter(1.0, 0.0)
    _check(img, [(P, u, 3.0, False)], [0])


@pytest.mark.parametrize("hw", [(16, 16), (8, 24), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_diffjpeg(hw):
    img = _image(*hw)
    for q in QUALITIES:
        lq = _check(img, [(J, q)], [0])
        assert not np.array_equal(lq, img)
    _check(img, [(G, _normal(img.shape), 25.0, False), (J, 40.25), (J, 70.5)], [1, 2])   # two in a row, on floats that are no bytes


@pytest.mark.parametrize("back_first", [True, False], ids=["resize_sinc_jpeg", "jpeg_resize_sinc"])
def test_both_final_orders(back_first):
    """The recipe's whole shape, by hand, on 67 x 90: stage 1, stage 2, one of the two final orders, bicubic back."""
    h, w = 67, 90
    s2h, s2w = h // 4, w // 4
    sinc = D.circular_lowpass_kernel(2.1, 9, 21)
    l1 = (int(np.floor(h * 0.7)), int(np.floor(w * 0.7)))
    ops = [(F, _kernel(21)), (R, LIN, l1[0], l1[1], 0.7), (P, _uniform(l1), 1.5, True), (J, 61.25), (F, _kernel(21)), (R, AREA, 14, 19, 0.0),
           (G, _normal((14, 19, 3)), 9.0, False)]
    tail = [(R, CUB, s2h, s2w, 0.0), (F, sinc)]
    ops += tail + [(J, 33.75)] if back_first else [(J, 33.75)] + tail
    ops.append((R, CUB, h, w, 0.0))
    _check(_image(h, w), ops, list(range(len(ops))))


def _drawable(rec, h, w, seed):
    for i in range(100):
        try:
            return f"g{i}.png", D.draw(rec, f"g{i}.png", h, w, seed)
        except D.DegradeError:
            continue
    raise AssertionError("no file name draws a chain at this size")


@pytest.mark.parametrize("hw", [(48, 64), (67, 90), (128, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_drawn_chains(hw):
    h, w = hw
    _, p = _drawable(D.load_recipe("realesrgan"), h, w, h)
    print(f"{h} x {w}: {p.describe()}")
    _check(_image(h, w), list(p.ops), list(range(len(p.ops))))


# ---------------------------------------------------------------- the ABI's conventions
def _three():
    h, w = 48, 64
    rec = D.load_recipe("realesrgan")
    imgs = [_image(h, w, s) for s in (0, 1, 2)]
    ps = [_drawable(rec, h, w, s)[1] for s in (10, 11, 12)]
    return h, w, imgs, ps


def test_a_batch_equals_its_images_run_singly_and_a_second_call():
    h, w, imgs, ps = _three()
    lq = D.degrade_chain(_ctx(), imgs, ps)
    for i in range(3):
        assert np.array_equal(lq[i], D.degrade_chain(_ctx(), [imgs[i]], [ps[i]])[0]), i
        assert np.array_equal(lq[i], M.degrade_chain_model(imgs[i], ps[i].ops)), i
    again = D.degrade_chain(_ctx(), imgs, ps)
    assert all(np.array_equal(a, b) for a, b in zip(lq, again))


def _staged(ps, imgs, rows, pitch):
    """The images embedded in [n][rows][pitch] and the chains' arrays on the device -> (src, records, keep-alive)."""
    h, w = imgs[0].shape[:2]
    buf = np.random.default_rng(3).integers(0, 256, (len(imgs), rows, pitch), dtype=np.uint8)
    for k, img in enumerate(imgs):
        buf[k, :h, :3 * w] = img.reshape(h, -1)
    host = np.zeros(sum(D.extra_bytes(p) for p in ps) + 256, dtype=np.uint8)
    at, offs = 0, []
    for p in ps:
        o, _, at = D.pack_extras(p, host, at)
        offs.append(o)
    dev = torch.from_numpy(host).cuda()
    tables = torch.from_numpy(D.chain_tables()).cuda()
    recs = [D.chain_record(p, dev.data_ptr(), o, tables.data_ptr()) for p, o in zip(ps, offs)]
    return torch.from_numpy(buf).cuda(), recs, (dev, tables)


def test_embedded_images_with_rows_and_pitch_and_exact_workspace():
    """rows > h and pitch > 3 w: the same bytes, nothing outside the h x w rectangles or behind the stated workspace is written."""
    ctx = _ctx()
    h, w, imgs, ps = _three()
    rows, pitch = h + 5, 3 * w + 29
    src, recs, keep = _staged(ps, imgs, rows, pitch)
    sizes = [D.check_chain(p, h, w) for p in ps]
    mh, mw = max(s[0] for s in sizes), max(s[1] for s in sizes)
    need = ctx.ws_bytes(L.STAGE_DEGRADE_CHAIN, 3, h, w, mh, mw)
    assert need == D.chain_ws_bytes(h, w, mh, mw) > 0
    out = torch.full((3, rows, pitch), CANARY, dtype=torch.uint8, device="cuda")
    raw = torch.full((need + 256 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    off = -raw.data_ptr() % 256
    ctx.check(ctx.lib.ir_degrade_chain(ctx.h, ctx.stream(), L.ptr(src), rows, pitch, 3, h, w, (L.Chain * 3)(*recs), L.ptr(out), None,
                                       C.c_void_p(raw.data_ptr() + off), need), "ir_degrade_chain")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k, :h, :3 * w].reshape(h, w, 3), M.degrade_chain_model(imgs[k], ps[k].ops)), k
        assert np.all(got[k, h:] == CANARY) and np.all(got[k, :, 3 * w:] == CANARY)
    r = raw.cpu().numpy()
    assert np.all(r[:off] == CANARY) and np.all(r[off + need:] == CANARY), "bytes outside the stated workspace were written"


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    h, w = 48, 64
    img = _image(h, w)
    k21 = _kernel(21)
    p = D.ChainParams(((F, k21), (R, LIN, 24, 32, 0.5), (G, _normal((24, 32, 3)), 5.0, False), (P, _uniform((24, 32)), 1.0, True), (J, 50.5), (R, CUB, h, w, 0.0)))
    src, recs, keep = _staged([p], [img], h, 3 * w)
    out = torch.full((h * w * 3,), CANARY, dtype=torch.uint8, device="cuda")
    tap = torch.full((h * w * 3,), 7.0, dtype=torch.float32, device="cuda")
    need = D.chain_ws_bytes(h, w, h, w)
    raw = torch.full((need + 512,), CANARY, dtype=torch.uint8, device="cuda")
    ws = raw.data_ptr() + (-raw.data_ptr() % 256)

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(src), po=L.ptr(out), pw=ws, wsb=need, rec=True, edit=None):
        r = L.Chain.from_buffer_copy(recs[0])
        if edit:
            edit(r)
        arr = (L.Chain * 1)(r) if rec else None
        return ctx.lib.ir_degrade_chain(ctx.h, ctx.stream(), pi, rows, pitch, n, hh, ww, arr, po, L.ptr(tap), C.c_void_p(pw) if pw else None, wsb)

    def op(i, **change):
        def edit(r):
            for k, v in change.items():
                setattr(r.ops[i], k, v)
        return edit

    def top(**change):
        def edit(r):
            for k, v in change.items():
                setattr(r, k, v)
        return edit

    refused = {
        "null image": call(pi=None), "null output": call(po=None), "null workspace": call(pw=0), "null records": call(rec=False),
        "no images": call(n=0), "h above rows": call(rows=h - 1), "short pitch": call(pitch=3 * w - 1), "a side above 8192": call(ww=8193, pitch=3 * 8193),
        "17 ops": call(edit=top(n_ops=17)), "negative op count": call(edit=top(n_ops=-1)), "tap past the ops": call(edit=top(tap=6)), "tap below -1": call(edit=top(tap=-2)),
        "unknown kind": call(edit=op(2, kind=6)), "kind 0": call(edit=op(2, kind=0)), "unknown mode": call(edit=op(1, a=3)),
        "even filter": call(edit=op(0, a=20)), "filter above 21": call(edit=op(0, a=23)), "null kernel": call(edit=op(0, data=None)), "misaligned kernel": call(edit=op(0, data=recs[0].ops[0].data + 4)),
        "image too small for the filter": call(hh=10, rows=10, edit=op(5, b=10)), "null field": call(edit=op(2, data=None)), "null uniforms": call(edit=op(3, data=None)),
        "negative sigma": call(edit=op(2, s=-1.0)), "negative scale": call(edit=op(3, s=-0.5)), "no exp table": call(edit=top(exp_table=None)),
        "no basis": call(edit=top(dct_basis=None)), "factor 0": call(edit=op(4, s=0.0)), "empty resize": call(edit=op(1, b=0)), "resize above 8192": call(edit=op(1, c=8193)),
        "scale factor against the size": call(edit=op(1, b=25)), "negative scale factor": call(edit=op(1, s=-0.5)), "ends at another size": call(edit=op(5, b=h - 1)),
        "short workspace": call(wsb=need - 1), "misaligned workspace": call(pw=ws + 128, wsb=need),
        "workspace for a smaller intermediate": call(edit=lambda r: (setattr(r.ops[1], "b", 96), setattr(r.ops[1], "c", 128), setattr(r.ops[1], "s", 2.0))),
    }
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in refused.values()), {k: v for k, v in refused.items() if v != -1}
    assert bool((out == CANARY).all()) and bool((tap == 7.0).all()), "a refused call wrote to the output"
    assert bool((raw == CANARY).all()), "a refused call wrote to the workspace"
    assert b"ir_degrade_chain" in ctx.lib.ir_last_error(ctx.h)
    assert call(edit=top(tap=1)) == 0   # and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    want_lq, want_tap = M.degrade_chain_model(img, p.ops, tap=1)
    assert np.array_equal(out.cpu().numpy().reshape(h, w, 3), want_lq)
    assert np.array_equal(_bits(tap.cpu().numpy()[:24 * 32 * 3].reshape(24, 32, 3)), _bits(want_tap)) and bool((tap[24 * 32 * 3:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_chain_equals_a_run_on_the_models_lq_image():
    """process(resize=, degrade=[ChainParams]) at the smallest network size, one 64 x 64 ground truth: the LQ image handed to lq_sink is the
    model's, and the results and scores are those of a run that is fed that LQ image as a plain input."""
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    gt = _image(64, 64, 4)
    rec = D.load_recipe("realesrgan")
    _, p = _drawable(rec, 64, 64, 231)
    assert isinstance(p, D.ChainParams)
    geo = job_geometry((64, 64), 1, True, 64)
    box = []
    preds, st1, scores = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(gt, geo)], degrade=[p], lq_sink=box.append, gt=[gt], **kw)
    want = M.degrade_chain_model(gt, p.ops)
    assert len(box) == 1 and len(box[0]) == 1 and np.array_equal(box[0][0], want)
    assert not np.array_equal(want, gt)
    plain, plain1, plain_scores = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(want, geo)], gt=[gt], **kw)
    assert np.array_equal(preds[0], plain[0]) and np.array_equal(st1[0], plain1[0])
    assert scores == plain_scores
    first = D.draw(D.load_recipe("lq"), "a.png", 64, 64, 231)
    with pytest.raises(ValueError, match="one kind"):
        process(dit, None, 2, "wavelet", False, False, 64, 32, resize=[ResizeJob(gt, geo)] * 2, degrade=[p, first], **kw)


def test_process_stream_chain_in_batches():
    """Two batches (two files of different sizes, then one that is enlarged) through process_stream: every LQ image is the model's."""
    from instarevive_amd.pipeline import process_stream
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    rec = D.load_recipe("realesrgan")
    sizes = [[(50, 64), (64, 100)], [(64, 44)]]   # the first two reach one network input, 64 x 128, from different sizes
    gts = [[_image(h, w, 9) for h, w in row] for row in sizes]
    ps = [[_drawable(rec, h, w, 5 + b)[1] for h, w in row] for b, row in enumerate(sizes)]
    records = [[ResizeJob(g, job_geometry((g.shape[1], g.shape[0]), 1, True, 64)) for g in row] for row in gts]
    assert [r.geo.net_hw for r in records[0]] == [(64, 128), (64, 128)]
    box = []
    out = list(process_stream(dit, gts, "wavelet", False, False, 64, 32, return_stage1=False, resize=records, degrade=ps, lq_sink=box.append, **kw))
    assert len(out) == 2 and [len(b) for b in box] == [2, 1]
    for lqs, row, prow in zip(box, gts, ps):
        for lq, g, p in zip(lqs, row, prow):
            assert np.array_equal(lq, M.degrade_chain_model(g, p.ops))
    plain = list(process_stream(dit, gts, "wavelet", False, False, 64, 32, return_stage1=False, resize=[[ResizeJob(lq, r.geo) for lq, r in zip(lqs, row)]
                                                                                                       for lqs, row in zip(box, records)], **kw))
    for (a, _), (b, _) in zip(out, plain):
        assert all(np.array_equal(x, z) for x, z in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_degrade_realesrgan_saves_the_models_lq_and_scores_like_a_run_on_it(tmp_path):
    """inference.py --degrade realesrgan --save_lq on a ground-truth folder, then a plain run on the saved LQ folder with --gt: the LQ files
    hold the model's pixels for the chains the file names draw, and both runs write the same results and the same metrics."""
    import subprocess
    import sys
    from PIL import Image
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _decode_tree
    d = tmp_path
    _write_artifacts(d)
    for f in (d / "in").glob("**/*"):
        if f.is_file():
            f.unlink()
    files = {"a.png": _image(64, 80, 1), "sub/b.png": _image(96, 64, 2)}
    rec = D.load_recipe("realesrgan")

    def draws(seed):
        try:
            return {name: D.draw(rec, name, img.shape[0], img.shape[1], seed) for name, img in files.items()}
        except D.DegradeError:
            return None
    seed = next(s for s in range(70, 200) if draws(s))   # a seed under which neither file's second blur meets a side below 11
    for name, img in files.items():
        (d / "in" / name).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(img).save(d / "in" / name)

    def run(out, src, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / src), "--output",
               str(d / out), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    run("out_deg", "in", "--degrade", "realesrgan", "--degrade_seed", str(seed), "--save_lq", str(d / "lq"), "--metrics_out", str(d / "deg.csv"))
    for name, p in draws(seed).items():
        saved = np.asarray(Image.open(d / "lq" / name).convert("RGB"))
        assert np.array_equal(saved, M.degrade_chain_model(files[name], p.ops)), name
    run("out_plain", "lq", "--resize", "gpu", "--gt", str(d / "in"), "--metrics_out", str(d / "plain.csv"))
    a, b = _decode_tree(d / "out_deg"), _decode_tree(d / "out_plain")
    assert sorted(a) == sorted(b) and len(a) == 2 and all(np.array_equal(a[k], b[k]) for k in a)
    assert (d / "deg.csv").read_text() == (d / "plain.csv").read_text() and "psnr_y" in (d / "deg.csv").read_text()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", "x", "--input", str(d / "in"), "--output", str(d / "no"), "--degrade", "realesrgan",
                        "--show_lq"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode != 0 and "cannot be combined with --show_lq" in r.stderr, r.stderr[-500:]
