"""The device resampler (csrc/resample.hip) through the C ABI, the pipeline and the command line. Pillow is the reference and the arithmetic is
integer: every comparison is exact equality. No byte outside the destination's full_h x full_w rectangle may be written, its padding must
be zero, and the saved files of --resize gpu must hold the pixels of --resize host."""
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
from tests.support import resample_model as M
from tests.test_resample_cpu import CASES, CHECKER_CASES, checkerboard, noise, pil_resize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _device_plan(ctx, in_hw, out_hw, flt):
    return torch.from_numpy(M.plan(ctx.lib, *in_hw, *out_hw, flt)).cuda()


def _resample(imgs, out_hw, flt, full_hw=None, in_pitch=None, out_pitch=None, slack=256):
    """ir_resample_u8 on imgs [n][in_h][in_w][3], placed in a buffer of row pitch in_pitch whose other bytes hold noise; the destination
    [n][full_h][out_pitch] (+ slack bytes) is filled with a canary first. -> (rc, the destination [n][full_h][out_pitch], the slack).
    The workspace is given 16 bytes more than the call is told of, which must stay untouched."""
    ctx = _ctx()
    n, in_h, in_w, _ = imgs.shape
    full_h, full_w = full_hw or out_hw
    in_pitch, out_pitch = in_pitch or 3 * in_w, out_pitch or 3 * full_w
    src = np.random.default_rng(77).integers(0, 256, (n, in_h, in_pitch), dtype=np.uint8)
    src[:, :, :3 * in_w] = imgs.reshape(n, in_h, 3 * in_w)
    d_in = torch.from_numpy(src).cuda()
    d_out = torch.full((n * full_h * out_pitch + slack,), CANARY, dtype=torch.uint8, device="cuda")
    plan = _device_plan(ctx, (in_h, in_w), out_hw, flt)
    need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, n, in_h, out_hw[1], 0, 0, 0))
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.ir_resample_u8(ctx.h, ctx.stream(), L.ptr(d_in), n, in_h, in_w, in_pitch, L.ptr(d_out), out_hw[0], out_hw[1], full_h, full_w, out_pitch,
                                L.ptr(plan), L.ptr(ws), need)
    torch.cuda.synchronize()
    assert bool((ws[need:] == CANARY).all())
    out = d_out.cpu().numpy()
    return rc, out[:n * full_h * out_pitch].reshape(n, full_h, out_pitch), out[n * full_h * out_pitch:]


def _check(img, out_hw, flt):
    rc, out, tail = _resample(img[None], out_hw, flt)
    assert rc == 0 and np.all(tail == CANARY)
    assert np.array_equal(out[0].reshape(out_hw + (3,)), pil_resize(img, out_hw, flt))


@pytest.mark.parametrize("flt,in_hw,out_hw", CASES + [
    (M.BICUBIC, (512, 512), (2048, 2048)),     # the product shape of --sr_scale 4
    (M.LANCZOS, (1536, 2048), (71, 97)),       # a strong reduction: 129 coefficients per output sample
    (M.BICUBIC, (50, 50), (71, 50)),           # the horizontal pass is skipped
    (M.BICUBIC, (37, 53), (37, 53)),           # both are: a copy, as PIL's resize to the same size
])
def test_noise_equals_pillow(flt, in_hw, out_hw):
    _check(noise(*in_hw, seed=in_hw[1]), out_hw, flt)


@pytest.mark.parametrize("flt,in_hw,out_hw", CHECKER_CASES)
def test_checkerboard_equals_pillow_where_both_clamps_fire(flt, in_hw, out_hw):
    img = checkerboard(*in_hw)
    if flt == M.LANCZOS:
        img = np.kron(checkerboard(in_hw[0] // 4, in_hw[1] // 4)[:, :, 0], np.ones((4, 4), np.uint8))[:, :, None].repeat(3, 2)
    want = pil_resize(img, out_hw, flt)
    assert want.min() == 0 and want.max() == 255
    _check(np.ascontiguousarray(img), out_hw, flt)


@pytest.mark.parametrize("flt,out_hw", [(M.BICUBIC, (1040, 1552)), (M.LANCZOS, (261, 389)), (M.BICUBIC, (520, 1000)), (M.LANCZOS, (333, 776))])
def test_padding_is_zero_and_nothing_else_is_written(flt, out_hw):
    """A 520 x 776 rectangle of a wider-pitch buffer into a canary-filled destination with full = the next multiples of 64 and a pitch beyond
    3 * full_w (an odd one too, so that the byte-store path of unaligned rows runs)."""
    img = noise(520, 776, seed=4)
    full = tuple(v + -v % 64 for v in out_hw)
    want = pil_resize(img, out_hw, flt)
    for extra in (40, 41):
        rc, out, tail = _resample(img[None], out_hw, flt, full_hw=full, in_pitch=3 * 776 + 52, out_pitch=3 * full[1] + extra)
        assert rc == 0 and np.all(tail == CANARY)
        assert np.array_equal(out[0, :out_hw[0], :3 * out_hw[1]].reshape(out_hw + (3,)), want)
        assert not out[0, out_hw[0]:, :3 * full[1]].any() and not out[0, :, 3 * out_hw[1]:3 * full[1]].any()
        assert np.all(out[0, :, 3 * full[1]:] == CANARY)


def test_batch_of_three_equals_three_calls_and_pillow():
    imgs = np.stack([noise(45, 61, seed=s) for s in (1, 2, 3)])
    for flt, out_hw in ((M.BICUBIC, (130, 200)), (M.LANCZOS, (20, 33))):
        rc, out, tail = _resample(imgs, out_hw, flt, full_hw=(out_hw[0] + 3, out_hw[1] + 5))
        assert rc == 0 and np.all(tail == CANARY)
        for i in range(3):
            _, one, _ = _resample(imgs[i:i + 1], out_hw, flt, full_hw=(out_hw[0] + 3, out_hw[1] + 5))
            assert np.array_equal(one[0], out[i])
            assert np.array_equal(out[i, :out_hw[0], :3 * out_hw[1]].reshape(out_hw + (3,)), pil_resize(imgs[i], out_hw, flt))


def test_two_chained_calls_equal_pillows_two_resizes():
    """(40, 56) at --sr_scale 1.5, then auto_resize to 512, as job_geometry chains them: a uint8 image between the calls."""
    from instarevive_amd.resample import job_geometry
    geo = job_geometry((56, 40), 1.5, False, 512)
    assert len(geo.chain) == 2
    img = noise(40, 56, seed=6)
    pil, dev = Image.fromarray(img), img
    for k, (tw, th) in enumerate(geo.chain):
        pil = pil.resize((tw, th), Image.BICUBIC)
        full = geo.net_hw if k == 1 else (th, tw)
        rc, out, _ = _resample(dev[None], (th, tw), M.BICUBIC, full_hw=full)
        assert rc == 0
        padded = out[0].reshape(full + (3,))
        dev = np.ascontiguousarray(padded[:th, :tw])
    from instarevive_amd.utils import pad
    assert np.array_equal(padded, pad(np.array(pil), 64))


def test_two_calls_give_identical_bytes():
    img = noise(300, 300, seed=8)[None]
    a = _resample(img, (1200, 1200), M.BICUBIC)[1]
    b = _resample(img, (1200, 1200), M.BICUBIC)[1]
    assert np.array_equal(a, b)


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((16 * 16 * 3,), CANARY, dtype=torch.uint8, device="cuda")
    plan = _device_plan(ctx, (8, 8), (16, 16), M.BICUBIC)
    need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 1, 8, 16, 0, 0, 0))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")

    def call(i=img, n=1, in_h=8, in_w=8, in_pitch=24, o=out, out_h=16, out_w=16, full_h=16, full_w=16, out_pitch=48, p=plan, w=ws.data_ptr(), wb=need):
        return ctx.lib.ir_resample_u8(ctx.h, ctx.stream(), L.ptr(i), n, in_h, in_w, in_pitch, L.ptr(o), out_h, out_w, full_h, full_w, out_pitch, L.ptr(p),
                                      C.c_void_p(w), wb)

    assert call(i=None) == -1 and call(o=None) == -1 and call(p=None) == -1 and call(w=None) == -1
    assert call(n=0) == -1 and call(in_h=0) == -1 and call(in_w=0) == -1 and call(out_h=0) == -1 and call(out_w=0) == -1
    assert call(full_h=15) == -1 and call(full_w=15) == -1
    assert call(in_pitch=23) == -1 and call(out_pitch=47) == -1
    assert call(wb=need - 1) == -1 and call(w=ws.data_ptr() + 1) == -1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    # a plan of other sizes: the launch compares its header with the call and writes nothing
    assert call(p=_device_plan(ctx, (8, 8), (16, 12), M.BICUBIC), out_w=16) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _host_prepared(raw, geo):
    """What read_job() hands to process(): the PIL chain and the zero pad."""
    from instarevive_amd.utils import pad
    im = Image.fromarray(raw)
    for size in geo.chain:
        im = im.resize(size, Image.BICUBIC)
    return pad(np.array(im), 64)


def _host_final(pred, geo):
    """write_job()'s un-padding and resize back to the LQ size."""
    crop = pred[:geo.valid_hw[0], :geo.valid_hw[1]]
    return np.array(Image.fromarray(crop).resize(geo.lq_size, Image.LANCZOS))


def test_process_stream_resize_equals_the_host_path():
    """process_stream(resize=...) on the reduced models: two batches of three images that reach a 64 x 128 network input from different decoded
    sizes - enlarged once, enlarged twice (--sr_scale 1.5, then the short edge to 64), not resized at all. Predictions and stage-1 images
    must equal process_stream on host-prepared arrays followed by the host's crop + LANCZOS; with png= the files must decode to them."""
    from instarevive_amd.pipeline import process, process_stream
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.golden._det import det_input
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    spec = [[((40, 56), 1), ((48, 80), 1), ((64, 100), 1)], [((20, 30), 1.5), ((64, 128), 1), ((33, 50), 1.5)]]   # ((h, w), sr_scale)
    records = []
    for b, row in enumerate(spec):
        records.append([])
        for i, ((h, w), sr) in enumerate(row):
            raw = (det_input(700 + 3 * b + i, (h, w, 3)) * 255).numpy().astype(np.uint8)
            records[-1].append(ResizeJob(raw, job_geometry((w, h), sr, True, 64)))
    assert all(r.geo.net_hw == (64, 128) for row in records for r in row)
    assert [len(r.geo.chain) for r in records[0]] == [1, 1, 0] and [len(r.geo.chain) for r in records[1]] == [2, 0, 2]
    assert records[0][2].geo.lanczos is None and records[0][0].geo.lanczos == (56, 40)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    host_batches = [[_host_prepared(r.raw, r.geo) for r in row] for row in records]
    plain = list(process_stream(dit, host_batches, "wavelet", False, False, 64, 32, return_stage1=True, **kw))
    raws = [[r.raw for r in row] for row in records]
    dev = list(process_stream(dit, raws, "wavelet", False, False, 64, 32, return_stage1=True, resize=records, **kw))
    rects = [[(r.geo.lq_size[1], r.geo.lq_size[0]) for r in row] for row in records]
    coded = list(process_stream(dit, raws, "wavelet", False, False, 64, 32, return_stage1=True, resize=records, png=rects, **kw))
    assert len(plain) == len(dev) == len(coded) == 2
    for (hp, h1), (dp, d1), (zp, z1), row in zip(plain, dev, coded, records):
        for host, got, blob, rec in list(zip(hp, dp, zp, row)) + list(zip(h1, d1, z1, row)):
            want = _host_final(host, rec.geo)
            assert got.shape == want.shape and np.array_equal(got, want)
            assert isinstance(blob, bytes) and np.array_equal(np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")), want)
    # process() takes the same argument; without stage-1 images the second list is empty
    gp, g1 = process(dit, None, 1, "wavelet", False, False, 64, 32, return_stage1=False, resize=records[1], **kw)
    assert g1 == [] and all(np.array_equal(g, _host_final(hst, r.geo)) for g, hst, r in zip(gp, plain[1][0], records[1]))


# ---------------------------------------------------------------------------------------------------------------- command line
def _run_cli(d, out, sr_scale, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
           str(d / out), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
           "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "3", "--workers", "4", "--sr_scale", str(sr_scale), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from tests.test_png_gpu import _decode_tree
    return _decode_tree(d / out), r.stdout


def _same_trees(a, b, count):
    assert sorted(a) == sorted(b) and len(a) == count
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("sr_scale", [1, 1.5])
def test_cli_resize_gpu_writes_the_host_pixels(tmp_path, sr_scale):
    """The 17-file folder of five sizes of test_png_gpu.py, each way in a child process: --resize gpu must save the pixels of --resize host; with
    --png_encoder gpu next to it no file is left to the host encoder."""
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _five_size_folder
    d = tmp_path
    _write_artifacts(d)
    sizes = _five_size_folder(d)
    host, _ = _run_cli(d, "out_host", sr_scale, "--resize", "host")
    gpu, _ = _run_cli(d, "out_gpu", sr_scale, "--resize", "gpu")
    _same_trees(host, gpu, len(sizes))
    if sr_scale == 1:
        both, stdout = _run_cli(d, "out_both", sr_scale, "--resize", "gpu", "--png_encoder", "gpu")
        note = [ln for ln in stdout.splitlines() if "took the host encoder" in ln]
        assert len(note) == 1 and " 0 of 17 files " in note[0], stdout[-1500:]
        _same_trees(host, both, len(sizes))
