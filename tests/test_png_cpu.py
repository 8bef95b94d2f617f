"""Host side of the device PNG encoder without a GPU: the CPU statement of its format (tests/support/png_model.py) decodes in zlib and PIL,
wrap_png frames any zlib stream of filtered scanlines, the command line's default and eligibility rule, and the parts of the C ABI that need
no device (ir_png_bound, the workspace dry run, the argument checks)."""
import ctypes as C
import io
import os
import sys
import zlib
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from instarevive_amd.png import wrap_png
from tests.support import png_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _photo_like(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 17.0) * np.cos(yy / 23.0), 127 + 80 * np.sin((xx + yy) / 31.0), 127 + 100 * np.cos(xx / 9.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8)


CASES = {
    "photo": _photo_like(96, 128),
    "noise": np.random.default_rng(1).integers(0, 256, (50, 70, 3), dtype=np.uint8),
    "constant": np.full((40, 33, 3), 77, np.uint8),
    "one_pixel": np.array([[[1, 2, 3]]], np.uint8),
    "row_not_multiple_of_16": _photo_like(37, 53, 2),   # 3 * 53 + 1 = 160 is, 3 * 53 = 159 is not; with 35 below neither
    "narrow": _photo_like(35, 11, 3),
}


def _open(png: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB"
    return np.asarray(im)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("rows", [8, 16, 64])
def test_model_decodes_in_zlib_and_pil(name, rows):
    img = CASES[name]
    z = M.encode(img, rows)
    assert zlib.decompress(z) == M.paeth_filter(img).tobytes()
    assert np.array_equal(_open(wrap_png(z, img.shape[1], img.shape[0])), img)
    assert len(z) <= M.bound(img.shape[0], img.shape[1], rows)


def test_model_limits_code_lengths_and_never_exceeds_the_fixed_code():
    # a histogram whose Huffman tree is far deeper than 15: counts growing like Fibonacci numbers
    hist = [0] * 257
    a, b = 1, 1
    for s in range(40):
        hist[s] = a
        a, b = b, a + b
    hist[256] = 1
    lens = M.limited_lengths(hist)
    assert max(lens) <= 15 and max(M.huffman_lengths(hist)) > 15
    assert sum(2.0 ** -l for l in lens if l) <= 1.0 + 1e-12
    fixed = [8] * 255 + [9, 9]
    assert sum(f * l for f, l in zip(hist, lens)) <= sum(f * l for f, l in zip(hist, fixed))
    codes = M.canonical_codes(lens)
    used = [(format(c, f"0{l}b")[::-1]) for c, l in zip(codes, lens) if l]   # back to MSB-first strings
    assert len(set(used)) == len(used) and not any(x != y and y.startswith(x) for x in used for y in used)


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrap_png_frames_a_zlib_stream(name):
    img = CASES[name]
    for level in (1, 6):
        png = wrap_png(zlib.compress(M.paeth_filter(img).tobytes(), level), img.shape[1], img.shape[0])
        assert np.array_equal(_open(png), img)
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and png[12:16] == b"IHDR" and png[-8:-4] == b"IEND"
    with pytest.raises(ValueError):
        wrap_png(b"", 0, 1)


def test_parser_default_is_the_host_encoder(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"])
    assert inf.parse_args().png_encoder == "host"
    assert eval_batch.parse_args().png_encoder == "host"
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--png_encoder", "gpu"])
    assert inf.parse_args().png_encoder == "gpu" and eval_batch.parse_args().png_encoder == "gpu"
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--png_encoder", "fpga"])
    with pytest.raises(SystemExit):
        inf.parse_args()


def test_gpu_encoder_eligibility_and_batching(tmp_path):
    """A job goes to the GPU encoder exactly when write_job() would save a plain crop of the prediction; on the cases of test_host_cpu.py's
    read_job test. For every eligible case write_job()'s file must equal that crop, which is what makes the two encoders interchangeable."""
    sys.path.insert(0, ROOT)
    import inference as inf
    from tests.golden._det import det_input
    src = tmp_path / "in" / "sub"
    src.mkdir(parents=True)
    Image.fromarray((det_input(3, (40, 56, 3)) * 255).numpy().astype(np.uint8)).save(src / "x.png")
    Image.fromarray((det_input(4, (520, 600, 3)) * 255).numpy().astype(np.uint8)).save(src / "big.png")
    base = dict(input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=1, tiled=False, tile_size=512, use_center_crop=False,
                show_lq=False, disable_preprocess_model=False)
    cases = [
        ("x.png", {}, None),                                                          # below 512: auto_resize enlarged it, LANCZOS brings it back
        ("x.png", dict(sr_scale=2.0, tiled=True, tile_size=64), (80, 112)),          # --sr_scale 2, tiles of 64: the network sees the LQ size
        ("x.png", dict(sr_scale=2.0, tiled=True, tile_size=64, show_lq=True), None),  # --show_lq: a strip of panels
        ("x.png", dict(use_center_crop=True), (512, 512)),                            # centre crop: nothing removed or resized
        ("big.png", {}, (520, 600)),                                                  # plain, at least 512: un-padded only
        ("big.png", dict(show_lq=True), None),
    ]
    for name, extra, want in cases:
        args = Namespace(**dict(base, **extra))
        job = inf.read_job(str(src / name), 0, args)
        assert inf.png_rect(job, args) == want, (name, extra)
        if want:
            pred = np.random.default_rng(5).integers(0, 256, job.net_in.shape, dtype=np.uint8)
            inf.write_job(job, pred, None, args)
            assert np.array_equal(np.array(Image.open(job.save_path)), pred[:want[0], :want[1]])
            inf.write_png_file(job, wrap_png(M.encode(pred[:want[0], :want[1]]), want[1], want[0]))
            assert np.array_equal(np.array(Image.open(job.save_path)), pred[:want[0], :want[1]])
            os.remove(job.save_path)
            inf.write_png_file(job, (M.encode(pred[:want[0], :want[1]]), want[1], want[0]))   # the un-framed form, framed on the writer thread
            assert np.array_equal(np.array(Image.open(job.save_path)), pred[:want[0], :want[1]])
    # batches never mix the two kinds, and stay as they were without a key
    mk = lambda h, w, ok: inf.Job("p", None, np.zeros((h, w, 3), np.uint8), (), "yes" if ok else "")
    jobs = [mk(64, 64, True), mk(64, 64, True), mk(64, 64, False), mk(64, 64, False), mk(64, 64, True), mk(64, 128, True)]
    groups = list(inf.batches_of(jobs, 3, key=lambda j: bool(j.src)))
    assert [[bool(j.src) for j in g] for g in groups] == [[True, True], [False, False], [True], [True]]
    assert [len(g) for g in inf.batches_of(jobs, 3)] == [3, 2, 1]


def test_host_bound_note_follows_the_encoder():
    sys.path.insert(0, ROOT)
    import inference as inf
    px = 2048 * 2048
    assert "host-bound" in inf.host_keeps_up(7, px, None) and "--png_encoder gpu" in inf.host_keeps_up(7, px, None)
    assert inf.host_keeps_up(7, px, None, "gpu") == "" and inf.host_keeps_up(1, px, None, "gpu") == ""
    assert inf.host_keeps_up(16, px, None) == inf.host_keeps_up(16, px, None, "host")


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


def test_bound_and_workspace_need_no_gpu():
    L, lib = _library()
    noise = CASES["noise"]
    for h, w in [(1, 1), (3, 7), (50, 70), (520, 776), (2048, 2048)]:
        assert lib.ir_png_bound(h, w) == M.bound(h, w), (h, w)
        assert lib.ir_workspace_bytes(None, L.STAGE_PNG, 1, h, w, 0, 0, 0) > 0
    assert lib.ir_png_bound(50, 70) >= len(M.encode(noise)) > noise.size
    assert lib.ir_png_bound(0, 5) == 0 and lib.ir_workspace_bytes(None, L.STAGE_PNG, 0, 8, 8, 0, 0, 0) == 0
    one, three = (lib.ir_workspace_bytes(None, L.STAGE_PNG, n, 2048, 2048, 0, 0, 0) for n in (1, 3))
    assert three > 2 * one > 2 * lib.ir_png_bound(2048, 2048)
    assert lib.ir_abi_version() == 3


def test_encode_refuses_bad_arguments_without_a_gpu():
    L, lib = _library()
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is launched
    assert lib.ir_png_encode(None, None, fake, 1, 8, 8, 24, 8, 8, fake, 1 << 20, fake, fake, 1 << 30) == -1
    # a rectangle outside the image (no context can be made without a device, so the check behind the null-context one is pinned on the GPU:
    # tests/test_png_gpu.py::test_bad_arguments_are_refused_and_write_nothing)
    for vh, vw in ((9, 8), (8, 9), (0, 8), (8, 0)):
        assert lib.ir_png_encode(None, None, fake, 1, 8, 8, 24, vh, vw, fake, 1 << 20, fake, fake, 1 << 30) == -1
