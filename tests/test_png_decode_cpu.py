"""The definition of the device PNG decoder (tools/png_decode_model.py) against Pillow and zlib, PngSource's refusals, the ABI additions and the
command line's refusals. No GPU. Every comparison is byte equality. The files built here are what tests/test_png_decode_gpu.py decodes on the
device.

The corpus: colour types 0 / 2 / 4 / 6 x the sizes x photo crop / noise / flat x Pillow's levels 0 / 1 / 6 / 9 and optimize=True. The five small
sizes take the full product; of the two large ones, where the plain-Python model takes a third of a second per file, every colour type meets
every content and every level, and every content every level (the combinations whose three indices sum to a multiple of 3)."""
import io
import os
import re
import subprocess
import sys
import zlib
from functools import lru_cache

import numpy as np
import pytest
from PIL import Image

from instarevive_amd import png_decode as P
from tools import png_decode_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOTO = os.path.join(ROOT, "tests", "golden", "jpeg_photo_640x419.jpg")
SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (17, 23), (96, 96), (65, 300)]
MODES = {0: "L", 2: "RGB", 4: "LA", 6: "RGBA"}
CONTENTS = ("photo", "noise", "flat")
LEVELS = (dict(compress_level=0), dict(compress_level=1), dict(compress_level=6), dict(compress_level=9), dict(optimize=True))
SPAN = 1024   # the span the tables are compared at: small enough that the small-block files have an entry per block


@lru_cache(maxsize=None)
def _photo():
    return np.array(Image.open(PHOTO).convert("RGB"))


def content(kind: str, h: int, w: int, channels: int, seed: int = 0) -> np.ndarray:
    """uint8 [h][w][channels]: a crop of the photograph (alpha: a ramp with noise), noise, or one colour."""
    rng = np.random.default_rng(1000 * h + w + seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 40, 90, 128][:channels], dtype=np.uint8), (h, w, channels)).copy()
    crop = _photo()[100:100 + h, 200:200 + w]
    colour = crop if channels >= 3 else np.array(Image.fromarray(crop).convert("L"))[..., None]
    if channels in (2, 4):
        alpha = ((np.arange(w)[None, :] * 3 + np.arange(h)[:, None]) % 256 + rng.integers(0, 4, (h, w))).astype(np.uint8)[..., None]
        colour = np.concatenate([colour, alpha], axis=2)
    return np.ascontiguousarray(colour)


def pil_png(px: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(px[..., 0] if px.shape[2] == 1 else px, MODES[{1: 0, 3: 2, 2: 4, 4: 6}[px.shape[2]]]).save(buf, format="PNG", **kw)
    return buf.getvalue()


def pil_pixels(data: bytes) -> np.ndarray:
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


@lru_cache(maxsize=None)
def corpus():
    """[(label, file bytes)] (shared, read-only)."""
    out = []
    for (h, w) in SIZES:
        for ci, ct in enumerate(MODES):
            for ki, kind in enumerate(CONTENTS):
                for li, kw in enumerate(LEVELS):
                    if h * w > 1000 and (ci + ki + li) % 3:
                        continue
                    px = content(kind, h, w, P.BPP[ct])
                    out.append((f"{h}x{w} type {ct} {kind} {'optimize' if 'optimize' in kw else 'level %d' % kw['compress_level']}", pil_png(px, **kw)))
    return out


def _noise(h, w, c, seed=5):
    return content("noise", h, w, c, seed)


def stored_of_deflate() -> bytes:
    """A level-0 stream whose payload is three copies of a memLevel=1 deflate stream: valid-looking dynamic headers that are not on the chain."""
    inner = M.deflate(M.filter_rows(content("photo", 96, 96, 3), [4] * 96), 6, 1)
    payload = np.frombuffer(inner * 3, dtype=np.uint8)
    return M.write_png(payload.reshape(1, -1, 1), [0], level=0)


def fixed_with_far_copy() -> bytes:
    """By the bit writer: a stored block of 32 768 bytes, then a fixed-Huffman block with two literals and a copy of 258 bytes at distance 32 768.
    Grey, 2 rows of 16 513 pixels: 33 028 inflated bytes."""
    w = 16513
    raw = bytearray(np.random.default_rng(9).integers(0, 256, 32768, dtype=np.uint8).tobytes())
    raw[0] = 0
    raw[w + 1] = 2   # the second row's filter type
    raw += bytes([7, 9])
    raw += raw[2:260]
    bw = M.BitWriter()
    bw.stored(bytes(raw[:32768]))
    bw.put(1, 1)
    bw.put(1, 2)
    bw.fixed_symbol(7)
    bw.fixed_symbol(9)
    bw.fixed_match(258, 32768)
    bw.fixed_symbol(256)
    assert len(raw) == 2 * (w + 1)
    return M.png_of_stream(2, w, 0, bw.zlib_stream(bytes(raw)))


@lru_cache(maxsize=None)
def hand_files():
    """[(label, file bytes)] written by the model's PNG writer (shared, read-only)."""
    rng = np.random.default_rng(3)
    out = []
    for c in (1, 2, 3, 4):
        px = content("photo", 23, 31, c)
        for t in range(5):
            out.append((f"filter {t} on every row, {c} bytes a pixel", M.write_png(px, [t] * 23)))
        out.append((f"the five filters cycling, {c} bytes a pixel", M.write_png(px, [y % 5 for y in range(23)])))
        out.append((f"random filters, {c} bytes a pixel", M.write_png(_noise(23, 31, c), rng.integers(0, 5, 23).tolist())))
    photo = content("photo", 96, 96, 3)
    paeth = [4] * 96
    out.append(("memLevel 1", M.write_png(photo, paeth, mem_level=1)))
    out.append(("full flush every 1000 bytes", M.write_png(np.concatenate([photo[:48], _noise(24, 96, 3), content("flat", 24, 96, 3)]), paeth, flush_every=1000)))
    out.append(("Z_FIXED", M.write_png(photo, paeth, strategy=zlib.Z_FIXED)))
    out.append(("Z_HUFFMAN_ONLY", M.write_png(photo, paeth, strategy=zlib.Z_HUFFMAN_ONLY)))
    # black, filter None: 90 100 equal bytes, which Z_RLE (distance 1 alone) codes as one chain of copies, each byte from the one before
    out.append(("Z_RLE constant 300 x 100", M.write_png(np.zeros((100, 300, 3), dtype=np.uint8), [0] * 100, strategy=zlib.Z_RLE)))
    out.append(("IDAT of 1 byte", M.write_png(photo[:20, :20], [4] * 20, idat=1)))
    out.append(("IDAT of 64 KB", M.write_png(_noise(200, 200, 3), [1] * 200, idat=65536, level=1)))
    out.append(("fixed block with a 258 copy at 32768", fixed_with_far_copy()))
    out.append(("stored stream of deflate bytes", stored_of_deflate()))
    return out


def source_of(data: bytes) -> P.PngSource:
    src, why = P.PngSource.open(data)
    assert src is not None, why
    return src


@lru_cache(maxsize=None)
def model_of(data: bytes, span_bits: int = SPAN):
    return M.decode(source_of(data), span_bits)


def inflated(src: P.PngSource) -> bytes:
    return zlib.decompressobj().decompress(src.stream.tobytes())


# ---------------------------------------------------------------------------------------------------------------- the model
def _check(label, data, span_bits=SPAN):
    src, r = source_of(data), model_of(data, span_bits)
    assert r["error"] == 0, label
    assert r["bytes"].tobytes() == inflated(src), f"{label}: the inflated bytes are not zlib's"
    assert np.array_equal(r["pixels"], pil_pixels(data)), f"{label}: the pixels are not Pillow's"
    return r


@pytest.mark.parametrize("h,w", SIZES)
def test_model_equals_pillow_and_zlib_on_pillows_files(h, w):
    files = [(lb, d) for lb, d in corpus() if lb.startswith(f"{h}x{w} ")]
    assert len(files) >= 20
    for label, data in files:
        _check(label, data)


def test_model_equals_pillow_and_zlib_on_hand_written_files():
    for label, data in hand_files():
        _check(label, data)


def test_model_is_the_same_at_the_smallest_and_largest_span():
    for label in ("memLevel 1", "full flush every 1000 bytes", "stored stream of deflate bytes"):
        data = dict(hand_files())[label]
        for span in (P.SPAN_MIN, P.SPAN_MAX):
            _check(label, data, span)


def test_the_inputs_cover_what_they_are_for():
    """True for the reference alone: these are statements about the files, not about the decoder."""
    runs = [model_of(d) for _, d in corpus() + hand_files()]
    kinds, types = set(), set()
    for r in runs:
        kinds |= {k for _, k in r["blocks"]}
        types |= set(r["types"].tolist())
    assert kinds == {0, 1, 2} and types == {0, 1, 2, 3, 4}
    hand = dict(hand_files())
    assert max(len(model_of(hand[k])["chain"]) for k in ("memLevel 1", "full flush every 1000 bytes")) >= 50
    r = model_of(hand["full flush every 1000 bytes"])
    assert {k for _, k in r["blocks"]} == {0, 1, 2}
    r = model_of(hand["stored stream of deflate bytes"], P.SPAN_MIN)
    on_chain = {s for s, _ in r["blocks"]}
    assert len([q for q in r["valid"].tolist() if q not in on_chain]) >= 1 and len(r["chain"]) == 1
    assert sum(1 for q in r["cand"].tolist() if q != P.NONE) >= 1
    assert model_of(hand["Z_RLE constant 300 x 100"])["rounds"] >= 12
    r = model_of(hand["fixed block with a 258 copy at 32768"])
    assert [k for _, k in r["blocks"]] == [0, 1] and int((np.arange(r["src0"].size) - r["src0"]).max()) == 32768


def corrupt_sources():
    """[(label, PngSource, error class)] for the device test: the model says each class first (it asserts every index in range)."""
    good = dict(hand_files())["memLevel 1"]
    out = []
    s = source_of(good)
    s.stream = s.stream[:(s.stream.size // 2) & ~3].copy()
    out.append(("truncated stream", s, M.E_PAST))
    s = source_of(good)
    s.adler ^= 1
    out.append(("flipped Adler", s, M.E_ADLER))
    raw = bytes(2 * 11)
    bw = M.BitWriter()
    bw.put(1, 1)
    bw.put(1, 2)
    bw.fixed_symbol(0)
    bw.fixed_match(21, 5)
    bw.fixed_symbol(256)
    out.append(("distance before the start", source_of(M.png_of_stream(2, 10, 0, bw.zlib_stream(raw))), M.E_DIST))
    bw = M.BitWriter()
    bw.put(1, 1)
    bw.put(1, 2)
    bw.fixed_symbol(0)
    bw.fixed_symbol(286)
    bw.fixed_symbol(256)
    out.append(("code that does not exist", source_of(M.png_of_stream(2, 10, 0, bw.zlib_stream(raw))), M.E_CODE))
    px = content("photo", 20, 20, 3)
    out.append(("wrong inflated size", source_of(M.png_of_stream(21, 20, 2, M.deflate(M.filter_rows(px, [1] * 20)))), M.E_SIZE))
    out.append(("filter byte 9", source_of(M.write_png(px, [1] * 10 + [9] + [2] * 9)), M.E_FILTER))
    return out


def test_corrupt_streams_have_their_error_class_in_the_model():
    for label, src, want in corrupt_sources():
        r = M.decode(src, SPAN)
        assert r["error"] == want and r["pixels"] is None, label


# ---------------------------------------------------------------------------------------------------------------- the host pass
def _refusals():
    px = content("photo", 8, 8, 3)
    good = M.write_png(px, [1] * 8)
    z = M.deflate(M.filter_rows(px, [1] * 8))
    buf = io.BytesIO()
    Image.fromarray(px).convert("P").save(buf, format="PNG")
    palette = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray((np.arange(64, dtype=np.uint16) * 900).reshape(8, 8)).save(buf, format="PNG")
    deep = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG", transparency=(1, 2, 3))
    trns = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG", save_all=True, append_images=[Image.fromarray(255 - px)])
    apng = buf.getvalue()
    at = good.index(b"IDAT") + 10
    crc = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
    wide = M.write_png(np.zeros((1, 70000, 1), dtype=np.uint8), [0])
    fixed = M.write_png(content("photo", 300, 300, 3), [1] * 300, strategy=zlib.Z_FIXED)
    assert len(fixed) > 70000
    return {
        "palette": palette, "depth": deep, "interlaced": M.png_of_stream(1, 1, 2, M.deflate(b"\0\1\2\3"), interlace=1), "transparency": trns,
        "animated": apng, "crc": crc, "size": wide, "short": M.png_of_stream(8, 8, 2, z[:5]), "fixed": fixed,
        "zlib": M.png_of_stream(8, 8, 2, bytes([z[0], z[1] ^ 1]) + z[2:]), "format": b"\xff\xd8" + good[2:], "truncated": good[:-6],
    }


def test_every_refusal_has_its_reason_and_the_file_takes_pillow():
    from argparse import Namespace
    import inference as cli
    files = _refusals()
    assert P.PngSource.open(M.write_png(content("photo", 300, 300, 3), [1] * 300, level=1))[0] is not None   # the same image in dynamic blocks
    assert P.PngSource.open(M.write_png(content("photo", 8, 8, 3), [1] * 8, strategy=zlib.Z_FIXED))[0] is not None    # fixed, but under 64 KB
    for reason, data in files.items():
        assert P.PngSource.open(data) == (None, reason), reason
    args = Namespace(resize_on_gpu=True, png_decode_log=[], use_center_crop=False, sr_scale=1, tiled=False, tile_size=512, save_format="png",
                     input="/in", output="/out")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for reason, data in files.items():
            path = os.path.join(d, reason + ".png")
            open(path, "wb").write(data)
            args.input = d
            try:
                want = np.array(Image.open(path).convert("RGB"))
            except Exception as e:   # what Pillow cannot read it cannot read behind the flag either: the same exception
                with pytest.raises(type(e)):
                    cli.decode_job(path, 0, args)
                continue
            job = cli.decode_job(path, 0, args)
            assert isinstance(job.raw, np.ndarray) and np.array_equal(job.raw, want), reason
    assert args.png_decode_log == list(files)


def test_source_holds_the_header_and_the_joined_stream():
    data = dict(hand_files())["IDAT of 1 byte"]
    src = source_of(data)
    assert src.shape == (20, 20, 3) and src.size == 1200 and src.color_type == 2 and src.inflated == 20 * 61 and src.stream.size % 4 == 0
    assert src.blob_bytes == src.stream.size and inflated(src) == M.filter_rows(content("photo", 96, 96, 3)[:20, :20], [4] * 20)
    assert src.adler == zlib.adler32(inflated(src))
    host = np.full(src.blob_bytes + 8, 7, dtype=np.uint8)
    src.pack(host, 4)
    assert np.array_equal(host[4:4 + src.blob_bytes], src.stream) and host[:4].tolist() == [7] * 4 and host[-4:].tolist() == [7] * 4


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_abi_additions():
    from instarevive_amd import _lib as L
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "instarevive_hip.h")).read())
    assert "IR_STAGE_PNG_DECODE = 25" in flat
    assert "int ir_png_decode(ir_ctx* ctx, void* stream, const ir_png_file* files, int n, int span_bits, uint32_t* info, void* ws, size_t ws_bytes);" in flat
    lib = L.load_library()
    assert lib.ir_abi_version() == 3 and L.STAGE_PNG_DECODE == 25 and "ir_png_decode" in L.SYMBOLS and hasattr(lib, "ir_png_decode")
    ws = lambda *a: int(lib.ir_workspace_bytes(None, L.STAGE_PNG_DECODE, *a))
    assert 0 < ws(1, 64, 64, 4096, 65536, 0) < ws(1, 64, 64, 4096, 256, 0) < ws(1, 128, 64, 4096, 256, 0) < ws(1, 128, 64, 65536, 256, 0)
    assert ws(1, 64, 64, 4096, 1024, 0) == ws(3, 64, 64, 4096, 1024, 0)   # the files of a batch share it
    for h, w, sb, span in ((64, 64, 4096, 65536), (1, 1, 8, 256), (100, 300, 123456, 1 << 20), (2049, 5, 4096, 1024)):
        assert ws(1, h, w, sb, span, 0) == P.layout(h, w, sb, span).total   # the sections the tests read lie where the library puts them
    for bad in ((1, 0, 64, 4096, 1024, 0), (1, 64, 65536, 4096, 1024, 0), (1, 64, 64, 4096, 128, 0), (1, 64, 64, 4096, 1 << 21, 0), (1, 64, 64, 4096, 1000, 0),
                (0, 64, 64, 4096, 1024, 0), (1, 64, 64, 4, 1024, 0), (1, 64, 64, 4098, 1024, 0), (1, 65535, 65535, 4096, 1024, 0)):
        assert ws(*bad) == 0, bad
    # without a GPU nothing can be launched, but every refusal comes first: null arguments are one
    assert lib.ir_png_decode(None, None, None, 1, 1024, None, None, 0) == -1
    assert lib.ir_png_decode(None, None, (L.PngFile * 1)(), 1, 1024, None, None, 0) == -1
    assert P.UNFILTER_LANES == 1024 and set(P.ERRORS) == set(range(1, 9))


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli(script, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), "--ckpt", "x", "--input", "in", "--output", "out", *flags],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("flag", ["--shard_tiles", "--show_lq", "--use_center_crop"])
def test_cli_refuses_the_flags_that_keep_the_resizes_on_the_host(flag):
    r = _cli("inference.py", "--png_decoder", "gpu", flag)
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--png_decoder gpu" in lines[0] and flag in lines[0], r.stderr[-1500:]


def test_eval_batch_takes_the_flag_and_refuses_gpu_without_the_device_crop():
    r = _cli("eval_batch.py", "--png_decoder", "gpu")
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1 and "--png_decoder gpu" in lines[0], r.stderr[-1500:]


def test_check_png_decoder_and_the_host_decoder_of_today(tmp_path):
    """--png_decoder host (the default): decode_job reads through PIL and holds the decoded array; gpu: a PNG becomes a PngSource with the header's
    size, anything PngSource refuses takes PIL, and the note counts both. With --jpeg_decoder gpu as well each file goes to its own decoder."""
    from argparse import Namespace
    import inference as cli
    from instarevive_amd.jpeg_decode import JpegSource
    os.makedirs(tmp_path / "in")
    px = content("photo", 96, 96, 3)
    Image.fromarray(px).save(tmp_path / "in" / "a.png")
    Image.fromarray(px).convert("P").save(tmp_path / "in" / "b.png")
    Image.fromarray(px).save(tmp_path / "in" / "c.jpg", quality=90)
    base = dict(save_format="png", input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=1, use_center_crop=False, tiled=False, tile_size=512,
                show_lq=False, shard_tiles=False, disable_preprocess_model=False, resize="gpu", resize_on_gpu=True)
    host = Namespace(**base, png_decoder="host")
    cli.check_png_decoder(host)
    assert not hasattr(host, "png_decode_log") and cli.png_decoder_note(host) == ""
    job = cli.decode_job(str(tmp_path / "in" / "a.png"), 0, host)
    assert isinstance(job.raw, np.ndarray) and np.array_equal(job.raw, px)
    gpu = Namespace(**{**base, "resize": "host"}, png_decoder="gpu")
    cli.check_png_decoder(gpu)
    assert gpu.resize == "gpu"
    jobs = [cli.decode_job(str(tmp_path / "in" / f), 0, gpu) for f in ("a.png", "b.png", "c.jpg")]
    assert isinstance(jobs[0].raw, P.PngSource) and jobs[0].raw.shape == px.shape and jobs[0].raw.size == px.size and jobs[0].geo == job.geo
    assert jobs[0].raw.name.endswith("a.png") and np.array_equal(M.decode(jobs[0].raw)["pixels"], px)
    assert all(isinstance(j.raw, np.ndarray) for j in jobs[1:])
    assert "1 of 3 files were decoded on the device, 2 took the host decoder (reasons: format: 1, palette: 1)" in cli.png_decoder_note(gpu)
    both = Namespace(**base, png_decoder="gpu", jpeg_decoder="gpu")
    cli.check_jpeg_decoder(both)
    cli.check_png_decoder(both)
    jobs = [cli.decode_job(str(tmp_path / "in" / f), 0, both) for f in ("a.png", "b.png", "c.jpg")]
    assert isinstance(jobs[0].raw, P.PngSource) and isinstance(jobs[1].raw, np.ndarray) and isinstance(jobs[2].raw, JpegSource)
    assert both.png_decode_log == [None, "palette"] and both.jpeg_decode_log == [None]
    for flag in ("show_lq", "use_center_crop", "shard_tiles"):
        with pytest.raises(SystemExit, match="--png_decoder gpu"):
            cli.check_png_decoder(Namespace(**{**base, flag: True}, png_decoder="gpu"))
    crop = Namespace(**{**base, "use_center_crop": True}, png_decoder="gpu", center_crop="gpu")
    cli.check_png_decoder(crop)   # accepted next to --center_crop gpu
    assert crop.png_decode_log == []
