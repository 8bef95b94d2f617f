"""The host side of --save_format jpg and the definition of ir_jpeg_encode, without a GPU: tools/jpeg_encode_model.py + instarevive_amd/jpeg.py's
wrap_jpeg against PIL's files, byte for byte; the header alone; the C ABI's additions; the command line's refusals and its host path."""
import ctypes as C
import io
import os
import re
import subprocess
import sys
from argparse import Namespace
from functools import lru_cache

import numpy as np
import pytest
from PIL import Image

from instarevive_amd.jpeg import RESTART_MCUS, jpeg_header, wrap_jpeg
from tools import degrade_folder as D
from tools.jpeg_encode_model import COUNTS, encode_model_counts, mcus_per_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (8, 9), (10, 16), (17, 23), (23, 17), (33, 70), (96, 272)]   # (h, w); 10 x 16: an even height that is no multiple of 16
QUALITIES = (1, 25, 75, 95, 100)


@lru_cache(maxsize=None)
def _content(h, w):
    rng = np.random.default_rng(1000 * h + w)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + yy * 2) // 2 % 256], -1).astype(np.uint8)
    for a in (noise, smooth):
        a.setflags(write=False)
    return noise, smooth


def content(h, w):
    """One noise and one smooth image of h x w from a seeded generator (shared, read-only)."""
    return list(_content(h, w))


def restarts_of(w, sub):
    """The restart intervals of the test set with PIL's arguments for them: 1, 5 (which divides no MCU count of the set but 1 x 5), the MCUs of
    one row, and a value above every MCU count."""
    row = mcus_per_row(w, sub)
    return [(1, dict(restart_marker_blocks=1)), (5, dict(restart_marker_blocks=5)), (row, dict(restart_marker_rows=1)), (5000, dict(restart_marker_blocks=5000))]


def pil_file(img, q, sub, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=q, subsampling=sub, **kw)
    return b.getvalue()


@pytest.mark.parametrize("h,w", SIZES)
def test_model_and_wrapper_equal_pils_file(h, w):
    for img in content(h, w):
        for q in QUALITIES:
            for sub in (0, 2):
                for restart, pil_kw in restarts_of(w, sub):
                    seg, _ = encode_model_counts(img, q, sub, restart)
                    assert wrap_jpeg(seg, w, h, q, sub, restart) == pil_file(img, q, sub, **pil_kw), (h, w, q, sub, restart)


def test_the_set_covers_every_rule():
    """From the model's counts: the set holds ZRL symbols, blocks with a non-zero 63rd coefficient, stuffed bytes, dummy blocks to the right
    and below, restart markers - and an even height that is no multiple of 16 under 4:2:0, the case edge rule 1 decides."""
    total = dict.fromkeys(COUNTS, 0)
    for h, w in SIZES:
        for img in content(h, w):
            for q in QUALITIES:
                for sub in (0, 2):
                    for k, v in encode_model_counts(img, q, sub, 5)[1].items():
                        total[k] += v
    print(total)
    assert all(total[k] > 0 for k in COUNTS), total
    assert any(h % 2 == 0 and h % 16 for h, _ in SIZES)
    # edge rule 1 decides it: replicating the full-resolution rows to 16 before the downsample gives other bytes for 10 x 16
    img = content(10, 16)[0]
    padded = np.pad(img, ((0, 6), (0, 0), (0, 0)), mode="edge")
    a, b = encode_model_counts(img, 75, 2, 5)[0], encode_model_counts(padded, 75, 2, 5)[0]
    assert a != b


def _split_header(blob):
    """(header through SOS, the rest) of a JPEG file."""
    at = blob.index(b"\xff\xda")
    at += 2 + int.from_bytes(blob[at + 2:at + 4], "big")
    return blob[:at], blob[at:]


@pytest.mark.parametrize("sub", [0, 2])
def test_header_equals_pils_and_the_file_decodes_to_the_roundtrip(sub):
    h, w = 33, 70
    img = content(h, w)[1]
    for q in (30, 95):
        want, _ = _split_header(pil_file(img, q, sub, restart_marker_blocks=RESTART_MCUS))
        assert jpeg_header(w, h, q, sub, RESTART_MCUS) == want
        seg, _ = encode_model_counts(img, q, sub, RESTART_MCUS)
        blob = wrap_jpeg(seg, w, h, q, sub, RESTART_MCUS)
        assert blob[:2] == b"\xff\xd8" and blob[-2:] == b"\xff\xd9"
        dec = Image.open(io.BytesIO(blob))
        assert dec.format == "JPEG" and dec.size == (w, h)
        if sub == 2:   # jpeg_roundtrip is the 4:2:0 pipeline
            assert np.array_equal(np.asarray(dec.convert("RGB")), D.jpeg_roundtrip(img, q))
    with pytest.raises(ValueError):
        jpeg_header(w, h, 0, sub, RESTART_MCUS)
    with pytest.raises(ValueError):
        jpeg_header(w, h, 95, 1, RESTART_MCUS)
    with pytest.raises(ValueError):
        jpeg_header(w, h, 95, sub, 65536)


def test_restart_interval_of_the_product():
    """A 2048 x 2048 result has several hundred intervals."""
    assert 200 <= (2048 // 16) ** 2 // RESTART_MCUS <= 2048


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_additions():
    from instarevive_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "IR_STAGE_JPEG = 18" in flat
    assert "size_t ir_jpeg_bound(int h, int w, int subsampling, int restart_mcus);" in flat
    assert ("int ir_jpeg_encode(ir_ctx* ctx, void* stream, const uint8_t* img, int n, int h, int w, long pitch, int vh, int vw, int quality, int subsampling, "
            "int restart_mcus, uint8_t* out, size_t out_stride, uint32_t* info, void* ws, size_t ws_bytes);") in flat
    lib = L.load_library()
    assert lib.ir_abi_version() == 3 and L.STAGE_JPEG == 18
    assert hasattr(lib, "ir_jpeg_bound") and hasattr(lib, "ir_jpeg_encode")
    b = lambda *a: int(lib.ir_jpeg_bound(*a))
    assert 0 < b(8, 8, 0, 1) < b(16, 16, 0, 1) < b(512, 512, 0, 32) < b(2048, 2048, 0, 32)
    assert 0 < b(16, 16, 2, 1) < b(17, 16, 2, 1) < b(17, 17, 2, 1)
    assert b(2048, 2048, 2, 32) < b(2048, 2048, 0, 32)
    for bad in ((0, 8, 2, 1), (8, 0, 2, 1), (8, 8, 1, 1), (8, 8, 2, 0), (8, 8, 2, 65536), (65536, 8, 2, 1)):
        assert b(*bad) == 0, bad
    # the bound holds the worst case per block - 20 DC bits and 63 x 26 AC bits, doubled for stuffing - and the markers
    assert b(8, 8, 0, 1) >= 2 * 3 * ((20 + 63 * 26 + 7) // 8)
    lib.ir_workspace_bytes.restype = C.c_size_t
    ws = lambda *a: int(lib.ir_workspace_bytes(None, L.STAGE_JPEG, *a))
    assert 0 < ws(1, 64, 64, 2, 32, 0) < ws(2, 64, 64, 2, 32, 0) and ws(1, 64, 64, 2, 32, 0) < ws(1, 64, 64, 0, 32, 0)
    assert ws(1, 64, 64, 1, 32, 0) == 0 and ws(1, 64, 64, 2, 0, 0) == 0
    # without a GPU nothing can be launched, but every refusal comes first: a null context is one
    assert lib.ir_jpeg_encode(None, None, None, 1, 8, 8, 24, 8, 8, 75, 2, 1, None, 0, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", "x", "--input", "in", "--output", "out", *flags],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("flags,word", [
    (("--save_format", "jpg", "--png_encoder", "gpu"), "--save_format jpg"),
    (("--save_format", "jpg", "--png_compress_level", "1"), "--save_format jpg"),
    (("--jpeg_quality", "90"), "--jpeg_quality"),
    (("--jpeg_subsampling", "444"), "--jpeg_subsampling"),
    (("--jpeg_encoder", "gpu"), "--jpeg_encoder"),
    (("--save_format", "jpg", "--jpeg_quality", "0"), "--jpeg_quality 0"),
])
def test_cli_refusals_are_one_line(flags, word):
    r = _cli(*flags)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and word in lines[0], r.stderr[-1500:]


def test_eval_batch_takes_the_same_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", "x", "--input", "in", "--output", "out", "--jpeg_encoder", "gpu"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--save_format jpg" in lines[0], r.stderr[-1500:]


@pytest.mark.parametrize("quality,subsampling", [(None, None), (60, "444")])
def test_host_path_writes_pils_bytes(tmp_path, quality, subsampling):
    """decode_job names the file <stem>_0.jpg and write_job's file is PIL's for the stated parameters and the product's restart interval."""
    import inference as cli
    os.makedirs(tmp_path / "in")
    src = content(96, 272)[1]
    Image.fromarray(src).save(tmp_path / "in" / "photo.png")
    args = Namespace(save_format="jpg", jpeg_quality=quality, jpeg_subsampling=subsampling, jpeg_encoder=None, png_encoder="host", png_compress_level=None,
                     input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=1, use_center_crop=True, tiled=False, tile_size=512, show_lq=False,
                     disable_preprocess_model=False)
    cli.check_save_format(args)
    assert (args.jpeg_quality, args.jpeg_subsampling, args.jpeg_encoder) == (quality or 95, subsampling or "420", "host")
    job = cli.decode_job(str(tmp_path / "in" / "photo.png"), 0, args)
    assert job.save_path == str(tmp_path / "out" / "photo_0.jpg")
    pred = content(512, 512)[1]
    cli.write_job(job, pred, None, args)
    want = pil_file(pred, quality or 95, {"420": 2, "444": 0}[subsampling or "420"], restart_marker_blocks=RESTART_MCUS)
    assert open(job.save_path, "rb").read() == want
    # the default format is untouched
    png = Namespace(**{**vars(args), "save_format": "png", "jpeg_quality": None, "jpeg_subsampling": None, "jpeg_encoder": None})
    cli.check_save_format(png)
    assert cli.decode_job(str(tmp_path / "in" / "photo.png"), 0, png).save_path.endswith("photo_0.png")
