"""The device PNG encoder (csrc/png_encode.hip) through the C ABI, the pipeline and both command lines: every file must decode in PIL to
exactly the pixels it was made from, no byte outside a stream may be written, and on photograph-like content the files must be no larger
than PIL's compress_level 1 files (tests/support/png_model.py, the CPU statement of the format, stays 10 - 18 % below that at every
chunk height from 8 to 64 rows, so the condition tests the coder and not the inputs)."""
import ctypes as C
import io
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from instarevive_amd.png import wrap_png
from tests.support import png_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _encode(buf: np.ndarray, vh: int, vw: int, slack: int = 64):
    """ir_png_encode on buf [n][h][w][3] -> (zlib streams, the whole output buffer, stride). The output buffer is filled with a canary first."""
    ctx = _ctx()
    n, h, w, _ = buf.shape
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    stride = int(ctx.lib.ir_png_bound(vh, vw)) + slack
    d_out = torch.full((n * stride + slack,), CANARY, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_PNG, n, vh, vw), dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_png_encode(ctx.h, ctx.stream(), L.ptr(d_img), n, h, w, 3 * w, vh, vw, L.ptr(d_out), stride, L.ptr(d_info), L.ptr(ws), ws.numel()),
              "ir_png_encode")
    torch.cuda.synchronize()
    out, sizes = d_out.cpu().numpy(), d_info.cpu().numpy().tolist()
    return [out[i * stride:i * stride + sizes[i]].tobytes() for i in range(n)], out, stride, sizes


def _check_round_trip(buf, vh, vw):
    streams, out, stride, sizes = _encode(buf, vh, vw)
    bound = stride - 64
    for i, z in enumerate(streams):
        want = np.ascontiguousarray(buf[i, :vh, :vw])
        assert 6 < sizes[i] <= bound, (sizes[i], bound)
        assert zlib.decompress(z) == M.paeth_filter(want).tobytes()
        got = np.asarray(Image.open(io.BytesIO(wrap_png(z, vw, vh))).convert("RGB"))
        assert got.shape == want.shape and np.array_equal(got, want)
        # nothing behind the stream's end, up to the next slot's first byte
        assert np.all(out[i * stride + sizes[i]:(i + 1) * stride] == CANARY), f"image {i}: bytes behind the stream's end were written"
    assert np.all(out[len(streams) * stride:] == CANARY)
    return streams


def _photo_like(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0 + seed) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w", [(2048, 2048), (64, 64), (1, 1), (3, 7)])
def test_round_trip_is_bit_exact(h, w):
    _check_round_trip(_photo_like(h, w, 3)[None], h, w)


def test_round_trip_of_a_valid_rectangle_in_a_padded_buffer():
    """520 x 776 of a 576 x 832 buffer: the pitch is not 3 * vw, and the padding's pixels must not reach the file."""
    buf = _photo_like(576, 832, 5)[None].copy()
    buf[:, 520:] = 255
    buf[:, :, 776:] = 0
    _check_round_trip(buf, 520, 776)


def test_round_trip_of_a_batch_of_three():
    buf = np.stack([_photo_like(200, 333, s) for s in (1, 2, 3)])
    streams = _check_round_trip(buf, 200, 333)
    assert len({len(z) for z in streams}) > 1 or streams[0] != streams[1]


def test_uniform_noise_stays_within_the_bound():
    rng = np.random.default_rng(9)
    buf = rng.integers(0, 256, (1, 300, 500, 3), dtype=np.uint8)
    streams, _, stride, sizes = _encode(buf, 300, 500)
    _check_round_trip(buf, 300, 500)
    raw = 300 * (3 * 500 + 1)
    print(f"uniform noise 300 x 500: {sizes[0]} bytes, bound {stride - 64}, filtered bytes {raw}, model {len(M.encode(buf[0]))}")
    assert sizes[0] <= stride - 64


def test_constant_image():
    _check_round_trip(np.full((1, 100, 120, 3), 77, np.uint8), 100, 120)
    _check_round_trip(np.zeros((1, 17, 5, 3), np.uint8), 17, 5)


def test_two_calls_give_identical_bytes():
    buf = _photo_like(512, 512, 8)[None]
    a, _, _, _ = _encode(buf, 512, 512)
    b, _, _, _ = _encode(buf, 512, 512)
    assert a == b


def _pil_size(img, level):
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=level)
    return len(b.getvalue())


@pytest.mark.parametrize("name", ["synthetic_a", "synthetic_b"])
def test_file_is_no_larger_than_pil_level_1(name):
    img = getattr(M, name)()
    assert img.shape == (1024, 1024, 3)
    streams = _check_round_trip(img[None], 1024, 1024)
    dev = len(wrap_png(streams[0], 1024, 1024))
    l1, l6, model = _pil_size(img, 1), _pil_size(img, 6), len(wrap_png(M.encode(img), 1024, 1024))
    print(f"{name}: device {dev} bytes = {dev / l1:.3f} of PIL level 1 ({l1}), {dev / l6:.3f} of level 6 ({l6}), {dev / model:.4f} of the model ({model})")
    assert dev <= l1


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    stride = int(ctx.lib.ir_png_bound(8, 8))
    out = torch.full((stride,), CANARY, dtype=torch.uint8, device="cuda")
    info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_PNG, 1, 8, 8), dtype=torch.uint8, device="cuda")
    call = lambda vh, vw, st, wsb, o=out: ctx.lib.ir_png_encode(ctx.h, ctx.stream(), L.ptr(img), 1, 8, 8, 24, vh, vw, L.ptr(o), st, L.ptr(info), L.ptr(ws), wsb)
    assert call(9, 8, stride, ws.numel()) == -1 and call(8, 0, stride, ws.numel()) == -1
    assert call(8, 8, stride - 1, ws.numel()) == -1 and call(8, 8, stride, ws.numel() - 1) == -1
    assert call(8, 8, stride, ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(info[0]) == -1
    assert call(8, 8, stride, ws.numel()) == 0


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_stream_png_decodes_to_the_arrays():
    """process_stream(png=...) on the reduced models: two batches, the second mixing two valid rectangles; predictions and stage-1 images must
    decode to exactly the crops of what png=None returns."""
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    batches = [[(det_input(500 + 2 * b + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(2)]
    rects = [[(64, 128), (64, 128)], [(40, 100), (64, 77)]]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    plain = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, **kw))
    coded = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, png=rects, **kw))
    assert len(plain) == len(coded) == 2
    for (preds, st1), (zp, z1), rr in zip(plain, coded, rects):
        for arr, blob, (vh, vw) in list(zip(preds, zp, rr)) + list(zip(st1, z1, rr)):
            assert isinstance(blob, bytes)
            got = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
            assert got.shape == (vh, vw, 3) and np.array_equal(got, arr[:vh, :vw])
    # process() takes the same argument; without stage-1 images the second list is empty
    zp, z1 = process(dit, batches[1], 1, "wavelet", False, False, 64, 32, return_stage1=False, png=rects[1], **kw)
    assert z1 == [] and all(np.array_equal(np.asarray(Image.open(io.BytesIO(b)).convert("RGB")), a[:r[0], :r[1]]) for b, a, r in zip(zp, plain[1][0], rects[1]))


def test_tile_sharded_frame_is_encoded_on_the_assembling_rank():
    """The --shard_tiles path: sharded_tiled_process(png=) makes the rank that assembles the frame encode it (HipTileEngine.blend_pixels(png=));
    the file must decode to the crop of the array the same call returns without png."""
    from instarevive_amd.parallel import sharded_tiled_process
    from instarevive_amd.pipeline import HipTileEngine
    from tests.golden._det import det_input
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    eng = HipTileEngine(dit, vae, sw, y.cuda(), mask3.cuda(), "wavelet", False, 64, 32)
    img = (det_input(77, (128, 192, 3)) * 255).numpy().astype(np.uint8)
    want, want1 = sharded_tiled_process(eng, [img], rank=0, world=1)
    got, got1 = sharded_tiled_process(eng, [img], rank=0, world=1, png=[(100, 150)])
    assert isinstance(got[0], bytes) and np.array_equal(got1[0], want1[0])
    dec = np.asarray(Image.open(io.BytesIO(got[0])).convert("RGB"))
    assert dec.shape == (100, 150, 3) and np.array_equal(dec, want[0][:100, :150])


# ---------------------------------------------------------------------------------------------------------------- command lines
def _decode_tree(folder):
    found = {}
    for root, _, names in os.walk(folder):
        for nm in names:
            found[os.path.relpath(os.path.join(root, nm), folder)] = np.array(Image.open(os.path.join(root, nm)).convert("RGB"))
    return found


def _five_size_folder(d):
    from tests.golden._det import det_input
    os.makedirs(d / "in" / "deep" / "er", exist_ok=True)
    sizes = [(64, 64), (40, 56), (64, 64), (64, 64), (33, 90), (64, 64), (40, 56), (72, 72), (64, 64), (64, 64), (50, 50), (64, 64), (64, 64), (40, 56),
             (512, 512), (512, 640), (600, 520)]   # the five sizes of test_cli_gpu.py (all enlarged by auto_resize) + three that are saved as plain crops
    for i, hw in enumerate(sizes):
        sub = ("", "deep/", "deep/er/")[i % 3]
        Image.fromarray((det_input(300 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / f"{sub}im{i:02d}.png")
    return sizes


def test_cli_gpu_encoder_writes_the_host_encoder_pixels(tmp_path):
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    sizes = _five_size_folder(d)
    outs = {}
    for enc in ("host", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
               str(d / f"out_{enc}"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "3", "--workers", "4", "--png_encoder", enc]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[enc] = _decode_tree(d / f"out_{enc}")
        if enc == "gpu":
            note = [ln for ln in r.stdout.splitlines() if "took the host encoder" in ln]
            assert len(note) == 1 and " 14 of 17 files " in note[0], r.stdout[-1500:]   # the fourteen small inputs are resized back by LANCZOS
    assert sorted(outs["host"]) == sorted(outs["gpu"]) and len(outs["host"]) == len(sizes)
    for k in outs["host"]:
        assert outs["host"][k].shape == outs["gpu"][k].shape and np.array_equal(outs["host"][k], outs["gpu"][k]), k


def test_eval_batch_gpu_encoder_writes_the_host_encoder_pixels(tmp_path):
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "lq" / "sub", exist_ok=True)
    srcs = {"a.png": (70, 90), "b.jpg": (64, 64), "sub/c.png": (150, 130), "d.png": (64, 100), "e.png": (97, 71)}
    for i, (k, hw) in enumerate(srcs.items()):
        Image.fromarray((det_input(80 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "lq" / k, quality=95)
    outs = {}
    for enc in ("host", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "lq"), "--output",
               str(d / f"res_{enc}"), "--cond_output", str(d / f"cond_{enc}"), "--batch_size", "2", "--image_size", "64", "--swinir_ckpt",
               str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
               "--prompt_embeds", str(d / "prompt.pth"), "--png_encoder", enc]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[enc] = (_decode_tree(d / f"res_{enc}"), _decode_tree(d / f"cond_{enc}"))
        if enc == "gpu":
            assert "0 of 10 files took the host encoder" in r.stdout, r.stdout[-1500:]
    for host, gpu in zip(outs["host"], outs["gpu"]):
        assert sorted(host) == sorted(gpu) and len(host) == len(srcs)
        for k in host:
            assert host[k].shape == gpu[k].shape == (64, 64, 3) and np.array_equal(host[k], gpu[k]), k
