"""The device PNG decoder (csrc/png_decode.hip) through the C ABI, the pipeline and the command line. Every check is byte equality: the pixels
against Pillow's np.array(Image.open(f).convert("RGB")), the chain table, the output offsets, the inflated bytes and info against
tools/png_decode_model.py. The files are those of tests/test_png_decode_cpu.py, where the model itself is held against Pillow and zlib and the
set's coverage is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from instarevive_amd import png_decode as P
from tests.test_png_decode_cpu import SIZES, SPAN, content, corpus, corrupt_sources, hand_files, model_of, pil_pixels, source_of
from tools import png_decode_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
GUARD = 4096


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _image(out, src):
    return out.cpu().numpy()[:, :3 * src.w].reshape(src.h, src.w, 3)


def _check_tables(label, data, src, ws, span=SPAN):
    t, r = P.tables(ws, src, span), model_of(data, span)
    assert t["error"] == r["error"] == 0, label
    for key in ("cand", "end", "next", "length", "status"):
        assert np.array_equal(t[key], r[key]), f"{label}: {key} differs from the model's"
    assert np.array_equal(t["chain"], r["chain"]) and t["total"] == r["total"], f"{label}: the chain differs from the model's"
    on = r["chain"]
    assert np.array_equal(t["offset"][on], r["offset"][on]), f"{label}: the output offsets differ from the model's"
    assert np.array_equal(t["src"], r["src"]) and np.array_equal(t["bytes"], r["bytes"]), f"{label}: the inflated bytes differ from the model's"
    assert t["adler"] == r["adler"], label


@pytest.mark.parametrize("h,w", SIZES)
def test_pillows_files_decode_to_pillows_pixels_and_the_models_tables(h, w):
    """All files of a size in one batch for the pixels, then each alone for the tables (a workspace holds its last file's)."""
    files = [(lb, d) for lb, d in corpus() if lb.startswith(f"{h}x{w} ")]
    sources = [source_of(d) for _, d in files]
    outs, info, _ = P.decode(_ctx(), sources, SPAN, fill=CANARY, guard=GUARD)
    assert info == [0] * len(files)
    for (label, data), src, out in zip(files, sources, outs):
        assert np.array_equal(_image(out, src), pil_pixels(data)), f"{label}: the pixels differ"
    for (label, data), src in list(zip(files, sources))[::3 if h * w < 1000 else 1]:
        outs, info, ws = P.decode(_ctx(), [src], SPAN, want_ws=True)
        assert info == [0] and np.array_equal(_image(outs[0], src), pil_pixels(data)), label
        _check_tables(label, data, src, ws)


def test_hand_written_files_decode_to_pillows_pixels_and_the_models_tables():
    for label, data in hand_files():
        src = source_of(data)
        outs, info, ws = P.decode(_ctx(), [src], SPAN, want_ws=True, fill=CANARY, guard=GUARD)
        assert info == [0], label
        assert np.array_equal(_image(outs[0], src), pil_pixels(data)), f"{label}: the pixels differ"
        _check_tables(label, data, src, ws)


@pytest.mark.parametrize("flt", [4, 3])
@pytest.mark.parametrize("h,w,c", [(P.UNFILTER_LANES + 77, 9, 3), (2 * P.UNFILTER_LANES + 1, 5, 4), (2 * P.UNFILTER_LANES + 1, 5, 1), (1500, 1, 2), (1, 1500, 3),
                                   (P.UNFILTER_LANES, 4, 3), (P.UNFILTER_LANES + 1, 4100, 1)])
def test_unfilter_shapes(h, w, c, flt):
    """All-Paeth and all-Average images around the unfilter workgroup's lane count: more rows than lanes, one row more than twice the lanes at
    width 5, width 1, height 1, exactly the lane count, and rows longer than the lanes are many (the schedule's other period)."""
    px = content("noise", h, w, c, seed=flt)
    data = M.write_png(px, [flt] * h, level=1)
    src = source_of(data)
    outs, info, _ = P.decode(_ctx(), [src], fill=CANARY, guard=GUARD)
    want = np.repeat(px[..., :1], 3, axis=2) if c < 3 else px[..., :3]
    assert info == [0] and np.array_equal(_image(outs[0], src), want)


def test_a_batch_equals_each_file_alone_twice_and_keeps_the_padding():
    hand = dict(hand_files())
    picks = [hand["memLevel 1"], hand["the five filters cycling, 1 bytes a pixel"], dict(corpus())["65x300 type 6 photo level 9"], hand["random filters, 2 bytes a pixel"]]
    sources = [source_of(d) for d in picks]
    assert len({(s.h, s.w) for s in sources}) >= 3 and {s.color_type for s in sources} == {0, 2, 4, 6}
    pitches = [3 * s.w + pad for s, pad in zip(sources, (5, 64, 1, 0))]
    first = P.decode(_ctx(), sources, pitches=pitches, fill=CANARY, guard=GUARD)
    again = P.decode(_ctx(), sources, pitches=pitches, fill=CANARY, guard=GUARD)
    assert first[1] == again[1] == [0, 0, 0, 0]
    for data, src, a, b in zip(picks, sources, first[0], again[0]):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(a, b)
        assert np.all(a[:, 3 * src.w:] == CANARY), "bytes between the rows were written"
        assert np.array_equal(a[:, :3 * src.w].reshape(src.h, src.w, 3), pil_pixels(data))
        alone, info, _ = P.decode(_ctx(), [src])
        assert info == [0] and np.array_equal(_image(alone[0], src), a[:, :3 * src.w].reshape(src.h, src.w, 3))


def test_pixels_do_not_depend_on_span_bits():
    hand = dict(hand_files())
    for label in ("memLevel 1", "full flush every 1000 bytes", "stored stream of deflate bytes", "IDAT of 64 KB"):
        src = source_of(hand[label])
        for span in (P.SPAN_MIN, P.SPAN_MAX):
            outs, info, ws = P.decode(_ctx(), [src], span, want_ws=True, fill=CANARY, guard=GUARD)
            assert info == [0] and np.array_equal(_image(outs[0], src), pil_pixels(hand[label])), (label, span)
            if label != "IDAT of 64 KB":   # the model's tables at these spans are those of the CPU test
                _check_tables(f"{label} at {span}", hand[label], src, ws, span)


def test_corrupt_streams_report_their_error_and_write_nothing_outside():
    """Each damaged stream next to a good file: info is the class the model gave, the good file is still Pillow's, and the guard bytes around every
    image and behind the workspace are intact (decode() asserts them)."""
    good_data = dict(hand_files())["the five filters cycling, 3 bytes a pixel"]
    for label, bad, want in corrupt_sources():
        assert M.decode(bad, SPAN)["error"] == want, label   # the model first: it asserts every index in range
        good = source_of(good_data)
        for span in (SPAN, P.SPAN_MAX):
            outs, info, ws = P.decode(_ctx(), [bad, good, bad], span, fill=CANARY, guard=GUARD, want_ws=True)
            assert info == [want, 0, want], (label, span)
            assert np.array_equal(_image(outs[1], good), pil_pixels(good_data)), label
            lay = P.layout(max(bad.h, good.h), max(bad.w, good.w), max(bad.stream.size, good.stream.size), span)   # the batch's sections
            assert P.tables(ws, bad, span, lay)["error"] == want


def test_bad_arguments_return_minus_one_and_write_nothing():
    ctx = _ctx()
    data = dict(hand_files())["the five filters cycling, 3 bytes a pixel"]
    src = source_of(data)
    host = torch.zeros((src.blob_bytes + 255) & ~255, dtype=torch.uint8)
    src.pack(host.numpy(), 0)
    dev = host.cuda()
    out = torch.full((src.h, 3 * src.w), CANARY, dtype=torch.uint8, device="cuda")
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    need = P.ws_bytes([src], 1024)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def call(rec, bits=1024, info_p=info.data_ptr(), ws_p=ws.data_ptr(), ws_n=need, n=1):
        return ctx.lib.ir_png_decode(ctx.h, ctx.stream(), (L.PngFile * 1)(rec), n, bits, info_p, ws_p, ws_n)

    rec = lambda **kw: src.record(dev.data_ptr(), out.data_ptr(), **kw)
    assert call(rec(), bits=128) == -1 and call(rec(), bits=1 << 21) == -1 and call(rec(), bits=1000) == -1
    assert call(rec(), ws_n=need - 1) == -1 and call(rec(), ws_p=ws.data_ptr() + 8) == -1 and call(rec(), ws_p=None) == -1
    assert call(rec(), info_p=None) == -1 and call(rec(), n=0) == -1
    assert call(rec(pitch=3 * src.w - 1)) == -1
    for field, value in (("stream", None), ("out", None), ("color_type", 3), ("color_type", 1), ("h", 0), ("w", 65536), ("stream_bytes", src.stream.size + 1),
                         ("stream_bytes", 4), ("stream", dev.data_ptr() + 2)):
        r = rec()
        setattr(r, field, value)
        assert call(r) == -1, field
    assert b"ir_png_decode" in ctx.lib.ir_last_error(ctx.h)
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == CANARY) and int(info[0]) == 77
    assert call(rec()) == 0
    torch.cuda.synchronize()
    assert int(info[0]) == 0 and np.array_equal(_image(out, src), pil_pixels(data))


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_takes_a_png_source_like_the_decoded_array():
    """process(resize=[ResizeJob(PngSource, geo)]) returns the bytes of the run on Pillow's decoded array, alone and together with degrade=."""
    from instarevive_amd import degrade as D
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_jpeg_gpu import _process_small
    dit, imgs, kw = _process_small()
    args = (1, "wavelet", False, False, 512, 448)
    rgba = np.concatenate([np.ascontiguousarray(imgs[0][:64, :64]), content("photo", 64, 64, 1)], axis=2)
    data = M.write_png(rgba, [y % 5 for y in range(64)], mem_level=1)
    src = source_of(data)
    pixels = pil_pixels(data)
    geo = job_geometry((64, 64), 1, True, 64)
    want = process(dit, None, *args, resize=[ResizeJob(pixels, geo)], **kw)
    got = process(dit, None, *args, resize=[ResizeJob(src, geo)], **kw)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[1][0], want[1][0])
    p = D.draw(D.load_recipe("lq"), "a/b.png", 64, 64, 231)
    box_a, box_b = [], []
    want = process(dit, None, *args, resize=[ResizeJob(pixels, geo)], degrade=[p], lq_sink=box_a.append, **kw)
    got = process(dit, None, *args, resize=[ResizeJob(src, geo)], degrade=[p], lq_sink=box_b.append, **kw)
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(box_a[0][0], box_b[0][0])
    # a stream the device cannot decode ends the batch with an error that names the file
    bad = source_of(data)
    bad.adler ^= 0x100
    bad.name = "broken.png"
    with pytest.raises(RuntimeError, match="broken.png"):
        process(dit, None, *args, resize=[ResizeJob(bad, geo)], **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_gpu_and_host_decoders_write_the_same_bytes(tmp_path):
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep", exist_ok=True)
    img = lambda i, hw: (det_input(700 + i, hw + (3,)) * 255).numpy().astype(np.uint8)
    Image.fromarray(img(0, (512, 512))).save(d / "in" / "a.png")
    Image.fromarray(img(1, (40, 56))).save(d / "in" / "deep" / "b.png", optimize=True)          # enlarged on the device
    Image.fromarray(img(2, (512, 576))[..., 0]).save(d / "in" / "c.png", compress_level=1)      # grey
    rgba = np.concatenate([img(3, (512, 512)), img(6, (512, 512))[..., :1]], axis=2)
    Image.fromarray(rgba).save(d / "in" / "d.png")                                              # alpha dropped
    Image.fromarray(img(4, (512, 512))).convert("P").save(d / "in" / "e.png")                   # palette: the host decoder
    px = img(5, (512, 512))
    open(d / "in" / "f.png", "wb").write(_adam7(px))                                            # interlaced: the host decoder
    assert np.array_equal(np.array(Image.open(d / "in" / "f.png").convert("RGB")), px)
    outs = {}
    for dec in ("host", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
               str(d / f"out_{dec}"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--workers", "2", "--resize", "gpu", "--png_decoder", dec]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[dec] = {os.path.relpath(os.path.join(root, nm), d / f"out_{dec}"): open(os.path.join(root, nm), "rb").read()
                     for root, _, names in os.walk(d / f"out_{dec}") for nm in names}
        note = [ln for ln in r.stdout.splitlines() if "--png_decoder gpu" in ln and "decoded on the device" in ln]
        if dec == "gpu":
            assert len(note) == 1, r.stdout[-1500:]
            assert " 4 of 6 files were decoded on the device, 2 took the host decoder (reasons: interlaced: 1, palette: 1)" in note[0], note[0]
        else:
            assert note == []
    assert sorted(outs["host"]) == sorted(outs["gpu"]) == ["a_0.png", "c_0.png", "d_0.png", "deep/b_0.png", "e_0.png", "f_0.png"]
    for k in outs["host"]:
        assert outs["host"][k] == outs["gpu"][k], k


def _adam7(px: np.ndarray) -> bytes:
    """An interlaced RGB file of px (Pillow does not write them): the seven passes, each filtered with None."""
    h, w, _ = px.shape
    raw = b""
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = px[y0::dy, x0::dx]
        if sub.size:
            raw += M.filter_rows(np.ascontiguousarray(sub), [0] * sub.shape[0])
    return M.png_of_stream(h, w, 2, M.deflate(raw), interlace=1)
