"""The device JPEG decoder (csrc/jpeg_decode.hip) through the C ABI, the pipeline and the command line. Every check is byte equality: the pixels
against Pillow's np.array(Image.open(f).convert("RGB")), the coefficients against tools/jpeg_decode_model.py. The files are those of
tests/test_jpeg_decode_cpu.py, where the model itself is held against Pillow and the set's coverage is asserted; the noise files at quality 100
hardly synchronise, so a decoder with a fixed number of rounds cannot pass them."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from instarevive_amd import jpeg_decode as J
from tests.test_jpeg_cpu import content
from tests.test_jpeg_decode_cpu import PHOTO, SIZES, coefficients_of, files_of, pil_jpeg, pil_pixels, plan_of
from tools import jpeg_decode_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _image(out, src):
    return out.cpu().numpy()[:, :3 * src.plan.w].reshape(src.plan.h, src.plan.w, 3)


@pytest.mark.parametrize("bits", [1024, 128])
@pytest.mark.parametrize("h,w", SIZES)
def test_pixels_equal_pillows_and_coefficients_the_models(h, w, bits):
    """All 42 files of a size in one batch: 4:4:4, 4:2:2, 4:2:0, grey, two restart layouts, standard and optimised tables, three qualities."""
    files = files_of(h, w)
    sources = [J.JpegSource(plan_of(d)) for _, d in files]
    outs, info, coefs = J.decode(_ctx(), sources, bits, want_coef=True)
    assert info == [0] * len(files)
    for (label, data), src, out, coef in zip(files, sources, outs, coefs):
        assert np.array_equal(coef, coefficients_of(data)[0]), f"{label} at {bits} bits: the coefficients differ (the entropy decode)"
        assert np.array_equal(_image(out, src), pil_pixels(data)), f"{label} at {bits} bits: the pixels differ (the back half)"


def test_the_stream_that_hardly_synchronises():
    """96 x 272 noise at quality 100, 4:4:4: one interval of more than 800 subsequences of 1024 bits that needs 85 rounds."""
    label, data = next((lb, d) for lb, d in files_of(96, 272) if lb.endswith("noise q100 444"))
    src = J.JpegSource(plan_of(data))
    assert len(src.intervals) == 1 and int(src.intervals[0, 1]) > 800 * 1024
    outs, info, coefs = J.decode(_ctx(), [src], 1024, want_coef=True)
    assert info == [0] and np.array_equal(coefs[0], coefficients_of(data)[0])
    assert np.array_equal(_image(outs[0], src), pil_pixels(data))


def test_photograph_equals_pillow():
    data = open(PHOTO, "rb").read()
    src = J.JpegSource(plan_of(data))
    outs, info, _ = J.decode(_ctx(), [src])
    assert info == [0] and np.array_equal(_image(outs[0], src), pil_pixels(data))


def test_writes_stay_inside_the_images_and_two_calls_agree():
    picks = [("17x23", "noise q75 420"), ("33x70", "smooth q100 422"), ("96x272", "noise q75 grey")]
    files = [next(d for lb, d in files_of(*map(int, size.split("x"))) if lb.endswith(tail)) for size, tail in picks]
    sources = [J.JpegSource(plan_of(d)) for d in files]
    pitches = [3 * s.plan.w + pad for s, pad in zip(sources, (5, 64, 1))]
    first = J.decode(_ctx(), sources, pitches=pitches, fill=CANARY)
    again = J.decode(_ctx(), sources, pitches=pitches, fill=CANARY)
    for data, src, a, b in zip(files, sources, first[0], again[0]):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b)
        assert np.all(a[:, 3 * src.plan.w:] == CANARY), "bytes between the rows were written"
        assert np.array_equal(a[:, :3 * src.plan.w].reshape(src.plan.h, src.plan.w, 3), pil_pixels(data))
    assert first[1] == again[1] == [0, 0, 0]


def test_device_encoder_round_trip():
    """What ir_jpeg_encode writes (4:4:4 and 4:2:0, restart 16), wrapped, decodes on the device to Pillow's decode of that file."""
    from instarevive_amd.jpeg import JpegEncoder
    ctx = _ctx()
    img = content(96, 272)[0]
    d_img = torch.from_numpy(img[None].copy()).cuda()
    for sub in (0, 2):
        enc = JpegEncoder(ctx, 1, 96, 272, 90, sub, 16)
        enc.queue(0, d_img, [(96, 272)])
        enc.fetch_sizes()
        torch.cuda.synchronize()
        blob = enc.fetch(1)[0]
        src, why = J.JpegSource.open(blob)
        assert src is not None, why
        assert src.plan.restart == 16 and len(src.intervals) > 1
        outs, info, _ = J.decode(ctx, [src])
        assert info == [0] and np.array_equal(_image(outs[0], src), pil_pixels(blob))


def test_malformed_streams_report_the_models_error_and_write_nothing_outside():
    """The same buffers with damaged contents: bits flipped in place, and a last interval cut one MCU short. info is the model's, the canary
    around the image is intact, and a valid call afterwards is right."""
    label, data = next((lb, d) for lb, d in files_of(33, 70) if lb.endswith("noise q75 420-restart5"))
    plan = plan_of(data)
    cases = []
    for seed in range(40):   # flips that the model says are an error, one per class met
        src = J.JpegSource(plan)
        rng = np.random.default_rng(seed)
        at = rng.integers(0, src.stream.size, 6)
        src.stream[at] ^= (1 << rng.integers(0, 8, 6)).astype(np.uint8)
        want = M.file_error(plan, (src.stream, src.intervals))
        if want and want not in [c[1] for c in cases]:
            cases.append((src, want))
    assert len(cases) >= 2, "the flips should meet more than one error class"
    src = J.JpegSource(plan)
    j = len(src.intervals) - 1
    off, cut = int(src.intervals[j, 0]), M.last_mcu_start(plan, j)
    bits = "".join(format(b, "08b") for b in src.stream[off:].tobytes())[:cut]
    bits += "1" * (-len(bits) % 8)
    src.stream[off:] = 0
    src.stream[off:off + len(bits) // 8] = np.frombuffer(int(bits, 2).to_bytes(len(bits) // 8, "big"), dtype=np.uint8)
    src.intervals[j, 1] = len(bits)
    assert M.file_error(plan, (src.stream, src.intervals)) == 4
    cases.append((src, 4))
    for bits_per in (1024, 128):
        outs, info, _ = J.decode(_ctx(), [c[0] for c in cases], bits_per, pitches=[3 * plan.w + 32] * len(cases), fill=CANARY)
        assert info == [c[1] for c in cases]
        for out in outs:
            assert np.all(out.cpu().numpy()[:, 3 * plan.w:] == CANARY)
    good = J.JpegSource(plan)
    outs, info, _ = J.decode(_ctx(), [good])
    assert info == [0] and np.array_equal(_image(outs[0], good), pil_pixels(data))


def test_bad_arguments_return_minus_one_and_write_nothing():
    ctx = _ctx()
    label, data = files_of(17, 23)[2]
    src = J.JpegSource(plan_of(data))
    host = torch.zeros((src.blob_bytes + 255) & ~255, dtype=torch.uint8)
    src.pack(host.numpy(), 0)
    dev = host.cuda()
    out = torch.full((src.plan.h, 3 * src.plan.w), CANARY, dtype=torch.uint8, device="cuda")
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    need = J.ws_bytes([src], 1024)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def call(rec, bits=1024, info_p=info.data_ptr(), ws_p=ws.data_ptr(), ws_n=need, n=1):
        arr = (L.JpegFile * 1)(rec)
        return ctx.lib.ir_jpeg_decode(ctx.h, ctx.stream(), arr, n, bits, info_p, None, ws_p, ws_n)

    rec = lambda **kw: src.record(dev.data_ptr(), out.data_ptr(), **kw)
    assert call(rec(), bits=96) == -1 and call(rec(), bits=8192) == -1 and call(rec(), bits=1000) == -1
    assert call(rec(), ws_n=need - 1) == -1 and call(rec(), ws_p=ws.data_ptr() + 8) == -1 and call(rec(), ws_p=None) == -1
    assert call(rec(), info_p=None) == -1 and call(rec(), n=0) == -1
    assert call(rec(pitch=3 * src.plan.w - 1)) == -1
    for field, value in (("stream", None), ("intervals", None), ("tables", None), ("out", None), ("hs", 3), ("comps", 2), ("n_intervals", 2), ("h", 7),
                         ("stream_bytes", src.stream.size + 1)):
        r = rec()
        setattr(r, field, value)
        assert call(r) == -1, field
    assert b"ir_jpeg_decode" in ctx.lib.ir_last_error(ctx.h)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == CANARY) and int(info[0]) == 77
    assert call(rec()) == 0
    torch.cuda.synchronize()
    assert int(info[0]) == 0 and np.array_equal(_image(out, src), pil_pixels(data))


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_takes_a_jpeg_source_like_the_decoded_array():
    """process(resize=[ResizeJob(JpegSource, geo)]) returns the bytes of the run on Pillow's decoded array, alone and together with degrade=."""
    from instarevive_amd import degrade as D
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_jpeg_gpu import _process_small
    dit, imgs, kw = _process_small()
    args = (1, "wavelet", False, False, 512, 448)
    data = pil_jpeg(np.ascontiguousarray(imgs[0][:64, :64]), quality=90)
    src, why = J.JpegSource.open(data)
    assert src is not None, why
    pixels = pil_pixels(data)
    geo = job_geometry((64, 64), 1, True, 64)
    want = process(dit, None, *args, resize=[ResizeJob(pixels, geo)], **kw)
    got = process(dit, None, *args, resize=[ResizeJob(src, geo)], **kw)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[1][0], want[1][0])
    p = D.draw(D.load_recipe("lq"), "a/b.jpg", 64, 64, 231)
    box_a, box_b = [], []
    want = process(dit, None, *args, resize=[ResizeJob(pixels, geo)], degrade=[p], lq_sink=box_a.append, **kw)
    got = process(dit, None, *args, resize=[ResizeJob(src, geo)], degrade=[p], lq_sink=box_b.append, **kw)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(box_a[0][0], box_b[0][0])
    # a stream the device cannot decode ends the batch with an error
    bad = J.JpegSource(src.plan)
    bad.stream[8:24] ^= 0x5A
    assert M.file_error(src.plan, (bad.stream, bad.intervals)) != 0
    bad.name = "broken.jpg"
    with pytest.raises(RuntimeError, match="broken.jpg"):
        process(dit, None, *args, resize=[ResizeJob(bad, geo)], **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_gpu_and_host_decoders_write_the_same_bytes(tmp_path):
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep", exist_ok=True)
    img = lambda i, hw: (det_input(700 + i, hw + (3,)) * 255).numpy().astype(np.uint8)
    Image.fromarray(img(0, (512, 512))).save(d / "in" / "a.jpg", quality=92)                                  # 4:2:0
    Image.fromarray(img(1, (40, 56))).save(d / "in" / "deep" / "b.jpg", quality=85, subsampling=0, optimize=True)   # 4:4:4, optimised tables; enlarged on the device
    Image.fromarray(img(2, (512, 576))[..., 0]).save(d / "in" / "c.jpg", quality=80)                           # grey
    Image.fromarray(img(3, (512, 512))).save(d / "in" / "d.jpg", quality=90, progressive=True)
    Image.fromarray(img(4, (512, 512))).save(d / "in" / "e.png")
    outs = {}
    for dec in ("host", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
               str(d / f"out_{dec}"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--workers", "2", "--resize", "gpu", "--jpeg_decoder", dec]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[dec] = {os.path.relpath(os.path.join(root, nm), d / f"out_{dec}"): open(os.path.join(root, nm), "rb").read()
                     for root, _, names in os.walk(d / f"out_{dec}") for nm in names}
        note = [ln for ln in r.stdout.splitlines() if "--jpeg_decoder gpu" in ln and "decoded on the device" in ln]
        if dec == "gpu":
            assert len(note) == 1 and " 3 of 5 files were decoded on the device, 2 took the host decoder" in note[0], r.stdout[-1500:]
        else:
            assert note == []
    assert sorted(outs["host"]) == sorted(outs["gpu"]) == ["a_0.png", "c_0.png", "d_0.png", "deep/b_0.png", "e_0.png"]
    for k in outs["host"]:
        assert outs["host"][k] == outs["gpu"][k], k
