"""The run mode of the device PNG encoder (ir_png_encode_runs, csrc/png_encode.hip) through the C ABI, the pipeline and the command line: on
every case of tests/support/png_runs_cases.py the stream decodes to the filtered bytes and the pixels, nothing outside it is written, it is
never longer than ir_png_encode's of the same buffer and exactly as long as the CPU model's (tests/support/png_runs_model.py: the code
lengths come from one deterministic construction, and every prefix code with the same lengths costs the same)."""
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
from tests.support import png_runs_cases as cases
from tests.support import png_runs_model as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
CORRECTNESS = cases.correctness_cases()


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _encode(buf: np.ndarray, vh: int, vw: int, runs: bool = True, slack: int = 64):
    """ir_png_encode_runs (or ir_png_encode) on buf [n][h][w][3] -> (zlib streams, the whole output buffer, stride, sizes). The output buffer is
    filled with a canary first."""
    ctx = _ctx()
    n, h, w, _ = buf.shape
    d_img = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    stride = int(ctx.lib.ir_png_bound(vh, vw)) + slack
    d_out = torch.full((n * stride + slack,), CANARY, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_PNG_RUNS if runs else L.STAGE_PNG, n, vh, vw), dtype=torch.uint8, device="cuda")
    name = "ir_png_encode_runs" if runs else "ir_png_encode"
    ctx.check(getattr(ctx.lib, name)(ctx.h, ctx.stream(), L.ptr(d_img), n, h, w, 3 * w, vh, vw, L.ptr(d_out), stride, L.ptr(d_info), L.ptr(ws), ws.numel()), name)
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
        assert np.all(out[i * stride + sizes[i]:(i + 1) * stride] == CANARY), f"image {i}: bytes behind the stream's end were written"
    assert np.all(out[len(streams) * stride:] == CANARY)
    return streams


@pytest.mark.parametrize("name", sorted(CORRECTNESS))
def test_round_trip_and_length(name):
    buf, vh, vw = CORRECTNESS[name]
    streams = _check_round_trip(buf, vh, vw)
    literal, _, _, _ = _encode(buf, vh, vw, runs=False)
    for i, (z, lit) in enumerate(zip(streams, literal)):
        model = len(R.encode(np.ascontiguousarray(buf[i, :vh, :vw])))
        print(f"{name}[{i}]: runs {len(z)}, literal-only {len(lit)}, model {model}")
        assert len(z) <= len(lit)
        assert len(z) == model
        if name == "noise":
            assert z == lit


def test_chunks_beyond_the_mask_capacity_stay_literal_only():
    """A chunk of more than 262144 filtered bytes (8 rows of 10923 pixels: 262160) has no room for its run marks in the LDS: the image takes
    ir_png_encode's launches and bytes. One pixel narrower (262136 bytes, the widest chunk the run mode codes) it is run-coded."""
    wide = np.full((1, 9, 10923, 3), 77, np.uint8)
    streams = _check_round_trip(wide, 9, 10923)
    assert streams == _encode(wide, 9, 10923, runs=False)[0]
    fits = np.ascontiguousarray(wide[:, :, :10922])
    streams = _check_round_trip(fits, 9, 10922)
    assert len(streams[0]) == len(R.encode(fits[0])) and 20 * len(streams[0]) < len(_encode(fits, 9, 10922, runs=False)[0][0])


def test_size_conditions_on_the_device():
    need = {"constant": 3.0, "sky": 3.0, "flat_regions": 3.0, "sky_over_photo": 1.15, "photo": 1.0}
    for name, img in cases.size_cases().items():
        z = _check_round_trip(img[None], 512, 512)[0]
        lit = _encode(img[None], 512, 512, runs=False)[0][0]
        print(f"{name}: runs {len(z)}, literal-only {len(lit)}: {len(lit) / len(z):.2f} times smaller")
        assert len(lit) >= need[name] * len(z), name


def test_two_calls_give_identical_bytes():
    img = cases.size_cases()["sky_over_photo"][None]
    assert _encode(img, 512, 512)[0] == _encode(img, 512, 512)[0]


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    stride = int(ctx.lib.ir_png_bound(8, 8))
    out = torch.full((stride,), CANARY, dtype=torch.uint8, device="cuda")
    info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_PNG_RUNS, 1, 8, 8), dtype=torch.uint8, device="cuda")
    call = lambda vh, vw, st, wsb, o=out: ctx.lib.ir_png_encode_runs(ctx.h, ctx.stream(), L.ptr(img), 1, 8, 8, 24, vh, vw, L.ptr(o), st, L.ptr(info), L.ptr(ws), wsb)
    assert call(9, 8, stride, ws.numel()) == -1 and call(8, 0, stride, ws.numel()) == -1
    assert call(8, 8, stride - 1, ws.numel()) == -1 and call(8, 8, stride, ws.numel() - 1) == -1
    assert call(8, 8, stride, ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(info[0]) == -1
    assert call(8, 8, stride, ws.numel()) == 0


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_stream_png_runs_decodes_to_the_arrays():
    """process_stream(png=..., png_runs=True) on the reduced models, as tests/test_png_gpu.py checks the default mode: the files decode to the
    crops of what a plain call returns, and none is larger than the default mode's file."""
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    batches = [[(det_input(500 + 2 * b + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)] for b in range(2)]
    rects = [[(64, 128), (64, 128)], [(40, 100), (64, 77)]]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    plain = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, **kw))
    lit = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, png=rects, **kw))
    coded = list(process_stream(dit, batches, "wavelet", False, False, 64, 32, return_stage1=True, png=rects, png_runs=True, **kw))
    assert len(plain) == len(coded) == 2
    for (preds, st1), (zp, z1), (lp, l1), rr in zip(plain, coded, lit, rects):
        for arr, blob, other, (vh, vw) in list(zip(preds, zp, lp, rr)) + list(zip(st1, z1, l1, rr)):
            assert isinstance(blob, bytes) and len(blob) <= len(other)
            got = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))
            assert got.shape == (vh, vw, 3) and np.array_equal(got, arr[:vh, :vw])
    zp, z1 = process(dit, batches[1], 1, "wavelet", False, False, 64, 32, return_stage1=False, png=rects[1], png_runs=True, **kw)
    assert z1 == [] and all(np.array_equal(np.asarray(Image.open(io.BytesIO(b)).convert("RGB")), a[:r[0], :r[1]]) for b, a, r in zip(zp, plain[1][0], rects[1]))
    assert {k[-1] for k in dit.ctx.__dict__["_png"]} == {False, True}   # the two modes took encoders of their own


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_png_runs_writes_the_host_encoder_pixels(tmp_path):
    """inference.py --png_encoder gpu --png_runs over the folder of tests/test_png_gpu.py's command-line test: the host encoder's pixels, as
    many files through the device as without the flag, and no file larger than without it."""
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _decode_tree, _five_size_folder
    d = tmp_path
    _write_artifacts(d)
    sizes = _five_size_folder(d)
    outs, notes = {}, {}
    for tag, extra in (("host", ["--png_encoder", "host"]), ("gpu", ["--png_encoder", "gpu"]), ("runs", ["--png_encoder", "gpu", "--png_runs"])):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
               str(d / f"out_{tag}"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "3", "--workers", "4"] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[tag] = _decode_tree(d / f"out_{tag}")
        notes[tag] = [ln for ln in r.stdout.splitlines() if "took the host encoder" in ln]
    assert len(notes["runs"]) == 1 and notes["runs"] == notes["gpu"] and " 14 of 17 files " in notes["runs"][0]
    assert sorted(outs["host"]) == sorted(outs["runs"]) and len(outs["host"]) == len(sizes)
    for k in outs["host"]:
        assert np.array_equal(outs["host"][k], outs["runs"][k]), k
        assert os.path.getsize(d / "out_runs" / k) <= os.path.getsize(d / "out_gpu" / k), k
