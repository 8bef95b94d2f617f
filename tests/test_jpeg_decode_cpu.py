"""The definition of the device JPEG decoder (tools/jpeg_decode_model.py) against Pillow, the parser's refusals, the byte pass, the parallel
entropy model against the sequential one, the ABI additions and the command line's refusals. No GPU. The set built here (SIZES x contents x
qualities x variants = 294 files) is what tests/test_jpeg_decode_gpu.py decodes on the device."""
import io
import os
import re
import struct
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
from PIL import Image

from instarevive_amd import jpeg_decode as J
from tests.test_jpeg_cpu import content
from tools import jpeg_decode_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = os.path.join(ROOT, "tests", "golden", "jpeg_photo_640x419.jpg")
SIZES = [(8, 8), (8, 9), (10, 16), (17, 23), (23, 17), (33, 70), (96, 272)]
QUALITIES = (1, 75, 100)
VARIANTS = {   # name -> (greyscale, Image.save keywords)
    "444": (False, dict(subsampling=0)),
    "422": (False, dict(subsampling=1)),
    "420": (False, dict(subsampling=2)),
    "420-optimize": (False, dict(subsampling=2, optimize=True)),
    "420-restart5": (False, dict(subsampling=2, restart_marker_blocks=5)),
    "422-restart-rows": (False, dict(subsampling=1, restart_marker_rows=1)),
    "grey": (True, dict()),
}


def pil_jpeg(img, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pil_pixels(data: bytes) -> np.ndarray:
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


@lru_cache(maxsize=None)
def files_of(h, w):
    """[(label, file bytes)] of one size: 2 contents x 3 qualities x 7 variants (shared, read-only)."""
    out = []
    for name, img in zip(("noise", "smooth"), content(h, w)):
        for q in QUALITIES:
            for variant, (grey, kw) in VARIANTS.items():
                src = np.ascontiguousarray(img[..., 1]) if grey else img
                out.append((f"{h}x{w} {name} q{q} {variant}", pil_jpeg(src, quality=q, **kw)))
    return out


@lru_cache(maxsize=None)
def plan_of(data: bytes):
    plan, why = J.parse(data)
    assert plan is not None, why
    return plan


@lru_cache(maxsize=None)
def coefficients_of(data: bytes):
    counts = {}
    coef = M.decode_coefficients(plan_of(data), counts)
    coef.setflags(write=False)
    return coef, counts


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("h,w", SIZES)
def test_model_equals_pillow(h, w):
    for label, data in files_of(h, w):
        plan = plan_of(data)
        assert (plan.h, plan.w) == (h, w)
        got = M.pixels_of(plan, coefficients_of(data)[0])
        want = pil_pixels(data)
        assert np.array_equal(got, want), f"{label}: {int(np.count_nonzero(got != want))} bytes differ from Pillow's"


def test_model_equals_pillow_on_the_photograph():
    data = open(PHOTO, "rb").read()
    plan = plan_of(data)
    assert (plan.h, plan.w, plan.comps, plan.hs, plan.vs, plan.restart) == (419, 640, 3, 2, 2, 0)
    assert np.array_equal(M.decode_pixels(plan), pil_pixels(data))


def test_the_set_covers_every_rule():
    total = {k: 0 for k in M.COUNTS}
    right = below = optimised = even_not_16 = 0
    for h, w in SIZES:
        for label, data in files_of(h, w):
            plan = plan_of(data)
            for k, v in coefficients_of(data)[1].items():
                total[k] += v
            my, mx = plan.mcu_grid
            right += mx * 8 * plan.hs > w
            below += my * 8 * plan.vs > h
            optimised += (1, 0) in plan.huff and plan.huff[(1, 0)][0] != [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
            even_not_16 += plan.comps == 3 and plan.vs == 2 and h % 2 == 0 and h % 16 != 0
    for k in M.COUNTS:   # ZRL, blocks that end at coefficient 63, stuffed bytes, restart markers, negative DC differences, codes beyond the first-level table
        assert total[k] > 0, k
    assert right > 0 and below > 0 and optimised > 0 and even_not_16 > 0


@pytest.mark.parametrize("h,w", SIZES)
def test_parallel_model_equals_the_sequential_one(h, w):
    for label, data in files_of(h, w):
        want = coefficients_of(data)[0]
        for bits in (128, 1024):
            got, rounds = M.parallel_entropy_model(plan_of(data), bits)
            assert np.array_equal(got, want), f"{label} at {bits} bits"


def test_the_set_holds_streams_that_synchronise_at_once_and_streams_that_hardly_do():
    """Correctness must not lean on quick synchronisation: the noise file at quality 100 needs more rounds than any fixed small number."""
    label, data = next((lb, d) for lb, d in files_of(96, 272) if lb.endswith("noise q100 444"))
    plan = plan_of(data)
    stream, table = J.entropy_segments(plan)
    assert len(table) == 1 and -(-int(table[0, 1]) // 1024) > 512   # one interval, several workgroups of 256 subsequences
    assert M.parallel_entropy_model(plan, 1024)[1] > 64
    _, small = files_of(8, 8)[0]
    assert M.parallel_entropy_model(plan_of(small), 1024)[1] == 0


# ---------------------------------------------------------------------------------------------------------------- the parser
def _with_segments(data: bytes, extra: bytes) -> bytes:
    """`extra` behind SOI."""
    return data[:2] + extra + data[2:]


def _seg(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def test_parser_refusals():
    img = content(33, 70)[1]
    cases = {"progressive": pil_jpeg(img, progressive=True), "colourspace": pil_jpeg(img, keep_rgb=True)}
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, format="JPEG")
    cases["components"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    cases["format"] = buf.getvalue()
    good = pil_jpeg(img, quality=75)
    cases["truncated"] = good[:good.index(b"\xff\xc0") + 7]   # cut inside SOF0
    for why, data in cases.items():
        assert J.parse(data) == (None, why), why
    for h, w in ((1, 1), (7, 40), (40, 7)):
        assert J.parse(pil_jpeg(content(40, 40)[1][:h, :w].copy())) == (None, "small")
    # a wrong RSTn number
    data = bytearray(pil_jpeg(img, quality=75, restart_marker_blocks=2))
    at = data.index(b"\xff\xd1")
    data[at + 1] = 0xD3
    assert J.parse(bytes(data)) == (None, "restart")
    assert J.parse(b"") == (None, "format") and J.parse(b"\xff\xd8\xff") == (None, "format")


def test_parser_takes_extra_segments_fill_bytes_and_trailing_bytes():
    img = content(33, 70)[0]
    data = pil_jpeg(img, quality=75, restart_marker_blocks=3)
    want = pil_pixels(data)
    noisy = _with_segments(data, _seg(0xE1, b"Exif\x00\x00" + bytes(40)) + _seg(0xFE, b"a comment") + b"\xff\xff" + _seg(0xEC, b"Ducky"))
    at = noisy.index(b"\xff\xd0")
    noisy = noisy[:at] + b"\xff\xff" + noisy[at:]          # fill bytes in front of a restart marker
    noisy = noisy[:-2] + b"\xff\xff\xd9" + b"trailing bytes \xff\xd8\xff\x00"   # and in front of EOI; bytes behind EOI
    plan, why = J.parse(noisy)
    assert plan is not None, why
    assert np.array_equal(M.decode_pixels(plan), want)
    assert np.array_equal(pil_pixels(noisy), want)


def test_vectorised_byte_pass_equals_the_loop():
    seen_stuffing = seen_restart = 0
    for h, w in SIZES:
        for label, data in files_of(h, w):
            plan = plan_of(data)
            a, b = J.entropy_segments(plan), M.entropy_segments_loop(plan)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == np.uint32, label
            assert len(a[0]) % 4 == 0 and np.all(a[1][:, 0] % 4 == 0)
            seen_stuffing += b"\xff\x00" in plan.scan
            seen_restart += len(a[1]) > 1
    assert seen_stuffing and seen_restart


def test_table_blob_decodes_every_code():
    """The kernel's two-level lookup, restated: every code of every table of an optimised file finds its symbol."""
    _, data = next((lb, d) for lb, d in files_of(96, 272) if lb.endswith("noise q100 420-optimize"))
    plan = plan_of(data)
    assert J.table_blob(plan).size == J.TABLE_BYTES
    for (cls, tid), (counts, vals) in plan.huff.items():
        lut, limit, valoff, sym = J.huffman_tables((counts, vals))
        code, k = 0, 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                v16 = code << (16 - l)
                e = int(lut[v16 >> 7])
                if e:
                    assert (e >> 8, e & 255) == (l, vals[k])
                else:
                    ll = next(x for x in range(10, 17) if v16 < limit[x])
                    assert ll == l and sym[(valoff[ll] + (v16 >> (16 - ll))) & 255] == vals[k]
                code, k = code + 1, k + 1
            code <<= 1


def test_malformed_streams_have_the_models_error_class():
    _, data = next((lb, d) for lb, d in files_of(33, 70) if lb.endswith("noise q75 420-restart5"))
    plan = plan_of(data)
    assert M.file_error(plan) == 0
    assert M.file_error(plan._replace(scan=plan.scan[:len(plan.scan) - 6], segments=None)) != 0   # the last interval cut short


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_additions():
    from instarevive_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert "IR_STAGE_JPEG_DECODE = 19" in flat and "#define IR_JPEG_DECODE_TABLE_BYTES 6176" in flat
    assert ("int ir_jpeg_decode(ir_ctx* ctx, void* stream, const ir_jpeg_file* files, int n, int subseq_bits, uint32_t* info, int16_t* coef_or_null, "
            "void* ws, size_t ws_bytes);") in flat
    lib = L.load_library()
    assert lib.ir_abi_version() == 3 and L.STAGE_JPEG_DECODE == 19 and "ir_jpeg_decode" in L.SYMBOLS and hasattr(lib, "ir_jpeg_decode")
    assert L.JPEG_DECODE_TABLE_BYTES == J.TABLE_BYTES == 6176
    ws = lambda *a: int(lib.ir_workspace_bytes(None, L.STAGE_JPEG_DECODE, *a))
    assert 0 < ws(1, 64, 64, 4096, 1024, 0) < ws(1, 64, 64, 4096, 128, 0) < ws(1, 128, 64, 4096, 128, 0) < ws(1, 128, 64, 65536, 128, 0)
    assert ws(1, 64, 64, 4096, 1024, 0) == ws(3, 64, 64, 4096, 1024, 0)   # the files of a batch share it
    for bad in ((1, 7, 64, 4096, 1024, 0), (1, 64, 64, 4096, 96, 0), (1, 64, 64, 4096, 8192, 0), (1, 64, 64, 4096, 1000, 0), (0, 64, 64, 4096, 1024, 0)):
        assert ws(*bad) == 0, bad
    # without a GPU nothing can be launched, but every refusal comes first: null arguments are one
    assert lib.ir_jpeg_decode(None, None, None, 1, 1024, None, None, None, 0) == -1
    rec = (L.JpegFile * 1)()
    assert lib.ir_jpeg_decode(None, None, rec, 1, 1024, None, None, None, 0) == -1


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli(script, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), "--ckpt", "x", "--input", "in", "--output", "out", *flags],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("flag", ["--shard_tiles", "--show_lq", "--use_center_crop"])
def test_cli_refuses_the_flags_that_keep_the_resizes_on_the_host(flag):
    r = _cli("inference.py", "--jpeg_decoder", "gpu", flag)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--jpeg_decoder gpu" in lines[0] and flag in lines[0], r.stderr[-1500:]


def test_eval_batch_takes_the_flag_and_refuses_gpu():
    r = _cli("eval_batch.py", "--jpeg_decoder", "gpu")
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--jpeg_decoder gpu" in lines[0], r.stderr[-1500:]


def test_host_decoder_is_the_code_of_today(tmp_path):
    """--jpeg_decoder host (the default): decode_job reads through PIL and holds the decoded array; gpu: a JPEG becomes a JpegSource with the
    header's size, anything the parser refuses takes PIL, and the note counts both."""
    from argparse import Namespace
    import inference as cli
    os.makedirs(tmp_path / "in")
    img = content(96, 272)[1]
    Image.fromarray(img).save(tmp_path / "in" / "a.jpg", quality=90)
    Image.fromarray(img).save(tmp_path / "in" / "b.jpg", quality=90, progressive=True)
    Image.fromarray(img).save(tmp_path / "in" / "c.png")
    base = dict(save_format="png", input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=1, use_center_crop=False, tiled=False, tile_size=512,
                show_lq=False, shard_tiles=False, disable_preprocess_model=False, resize="gpu", resize_on_gpu=True)
    host = Namespace(**base, jpeg_decoder="host")
    cli.check_jpeg_decoder(host)
    assert not hasattr(host, "jpeg_decode_log") and cli.jpeg_decoder_note(host) == ""
    want = np.array(Image.open(tmp_path / "in" / "a.jpg").convert("RGB"))
    job = cli.decode_job(str(tmp_path / "in" / "a.jpg"), 0, host)
    assert isinstance(job.raw, np.ndarray) and np.array_equal(job.raw, want)
    gpu = Namespace(**{**base, "resize": "host"}, jpeg_decoder="gpu")
    cli.check_jpeg_decoder(gpu)
    assert gpu.resize == "gpu"
    jobs = [cli.decode_job(str(tmp_path / "in" / f), 0, gpu) for f in ("a.jpg", "b.jpg", "c.png")]
    assert isinstance(jobs[0].raw, J.JpegSource) and jobs[0].raw.shape == want.shape and jobs[0].raw.size == want.size and jobs[0].geo == job.geo
    assert np.array_equal(M.decode_pixels(jobs[0].raw.plan), want)
    assert all(isinstance(j.raw, np.ndarray) for j in jobs[1:]) and np.array_equal(jobs[2].raw, img)
    assert "1 of 3 files were decoded on the device, 2 took the host decoder (reasons: format: 1, progressive: 1)" in cli.jpeg_decoder_note(gpu)
