"""The run mode of the device PNG encoder without a GPU: the CPU statement of its format (tests/support/png_runs_model.py) decodes in zlib and
PIL on every case of tests/support/png_runs_cases.py and is never longer than the literal-only model, the size conditions on the 512 x 512
cases, the parts of the C ABI that need no device, and the command lines' flag."""
import ctypes as C
import io
import os
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from instarevive_amd.png import wrap_png
from tests.support import png_model as M
from tests.support import png_runs_cases as cases
from tests.support import png_runs_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORRECTNESS = cases.correctness_cases()
_size_cache = {}


def _sizes():
    """name -> (image, literal-only model's bytes, run model's bytes), computed once."""
    if not _size_cache:
        for name, img in cases.size_cases().items():
            _size_cache[name] = (img, len(M.encode(img)), R.encode(img))
    return _size_cache


def _images(name):
    buf, vh, vw = CORRECTNESS[name]
    return [np.ascontiguousarray(buf[i, :vh, :vw]) for i in range(len(buf))]


def _check_stream(z, img):
    assert zlib.decompress(z) == M.paeth_filter(img).tobytes()
    im = Image.open(io.BytesIO(wrap_png(z, img.shape[1], img.shape[0])))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


@pytest.mark.parametrize("name", sorted(CORRECTNESS))
def test_model_decodes_and_is_never_longer(name):
    for img in _images(name):
        choices = []
        z = R.encode(img, choices=choices)
        _check_stream(z, img)
        lit = len(M.encode(img))
        assert len(z) <= lit <= M.bound(img.shape[0], img.shape[1])
        if name == "noise":
            assert not any(choices) and len(z) == lit and z == M.encode(img)
        elif name not in ("photo_64", "padded"):
            assert any(choices) and len(z) < lit


def test_parse_of_the_special_cases():
    """What the cases were built for: the diagonal's chunks are one run each, the wide constant's zero runs cross the 4096-byte tiles and split into
    258-pieces, and the one-row images hold zero runs with exactly the remainders asked for."""
    filt = M.paeth_filter(_images("diagonal")[0])
    assert np.all(filt == 4)
    lit, head, length = R.tokens(filt[:8].reshape(-1))
    assert lit.tolist() == [0] and length.tolist() == [258] * 3 + [8 * 121 - 1 - 3 * 258]
    filt = M.paeth_filter(_images("constant_8x1400")[0])
    lit, head, length = R.tokens(filt.reshape(-1))
    assert filt.shape[1] == 4201 and (length == 258).sum() >= 8 * 16 and any(h < 4096 < h + l for h, l in zip(head.tolist(), length.tolist()))
    for rest in cases.RUN_RESTS:
        data = M.paeth_filter(_images(f"one_row_{rest}")[0]).reshape(-1)
        lit, head, length = R.tokens(data)
        want = [258] * (rest // 258) + ([rest % 258] if rest % 258 >= R.MIN else [])
        assert length.tolist() == want * 2 and np.all(data[head] == 0), rest
        assert len(lit) + int(length.sum()) == len(data)


def test_length_symbols_are_rfc_1951s():
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    bits = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    sym, eb, extra = R.length_symbol(np.arange(3, 259))
    for length, s, e, x in zip(range(3, 259), sym.tolist(), eb.tolist(), extra.tolist()):
        assert 257 <= s <= 285 and e == bits[s - 257] and base[s - 257] + x == length and x < (1 << e)
    assert sum(2.0 ** -l for l in R.CL_LENS if l) == 1.0


def test_size_conditions_on_the_model():
    def pil(img, level):
        b = io.BytesIO()
        Image.fromarray(img).save(b, format="PNG", compress_level=level)
        return len(b.getvalue())
    ratio = {}
    for name, (img, lit, z) in _sizes().items():
        _check_stream(z, img)
        ratio[name] = lit / len(z)
        print(f"{name}: literal-only {lit}, runs {len(z)} ({ratio[name]:.2f} times smaller), as files: runs {len(wrap_png(z, 512, 512))}, "
              f"PIL level 1 {pil(img, 1)}, PIL level 6 {pil(img, 6)}")
    assert min(ratio["constant"], ratio["sky"], ratio["flat_regions"]) >= 3.0, ratio
    assert ratio["sky_over_photo"] >= 1.15 and ratio["photo"] >= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------- the C ABI without a device
def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


def test_abi_declares_and_exports_the_run_mode():
    L, lib = _library()
    header = open(os.path.join(ROOT, "include", "instarevive_hip.h")).read()
    flat = " ".join(header.split())
    assert "IR_STAGE_PNG_RUNS = 20" in flat
    assert "int ir_png_encode_runs(ir_ctx* ctx, void* stream, const uint8_t* img, int n, int h, int w, long pitch, int vh, int vw, uint8_t* out, size_t out_stride, uint32_t* info, void* ws, size_t ws_bytes);" in flat
    assert "ir_png_encode_runs" in L.SYMBOLS and L.STAGE_PNG_RUNS == 20 and hasattr(lib, "ir_png_encode_runs")
    assert lib.ir_abi_version() == 3


def test_workspace_needs_no_gpu():
    L, lib = _library()
    ws = lambda stage, n, h, w: int(lib.ir_workspace_bytes(None, stage, n, h, w, 0, 0, 0))
    for h, w in [(1, 1), (3, 7), (8, 1400), (520, 776), (2048, 2048), (8, 10923)]:
        assert ws(L.STAGE_PNG_RUNS, 1, h, w) > ws(L.STAGE_PNG, 1, h, w) > 0
    assert ws(L.STAGE_PNG_RUNS, 0, 8, 8) == 0 and ws(L.STAGE_PNG_RUNS, 1, 0, 8) == 0
    assert ws(L.STAGE_PNG_RUNS, 3, 2048, 2048) > 2 * ws(L.STAGE_PNG_RUNS, 1, 2048, 2048)


def test_encode_runs_refuses_bad_arguments_without_a_gpu():
    L, lib = _library()
    fake = C.c_void_p(0x1000)   # never dereferenced: every call below is refused before anything is launched
    assert lib.ir_png_encode_runs(None, None, fake, 1, 8, 8, 24, 8, 8, fake, 1 << 20, fake, fake, 1 << 30) == -1
    for vh, vw in ((9, 8), (8, 9), (0, 8), (8, 0)):
        assert lib.ir_png_encode_runs(None, None, fake, 1, 8, 8, 24, vh, vw, fake, 1 << 20, fake, fake, 1 << 30) == -1


# ---------------------------------------------------------------------------------------------------------------- command lines
def test_flag_is_off_by_default_and_needs_the_gpu_encoder(monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import eval_batch
    import inference as inf
    base = ["prog", "--ckpt", "c", "--input", "i", "--output", "o"]
    for mod in (inf, eval_batch):
        monkeypatch.setattr(sys, "argv", base)
        args = mod.parse_args()
        assert args.png_runs is False
        inf.check_save_format(args)
        monkeypatch.setattr(sys, "argv", base + ["--png_encoder", "gpu", "--png_runs"])
        args = mod.parse_args()
        assert args.png_runs is True and args.png_encoder == "gpu"
        inf.check_save_format(args)
        monkeypatch.setattr(sys, "argv", base + ["--png_runs"])
        with pytest.raises(SystemExit) as e:
            inf.check_save_format(mod.parse_args())
        assert "--png_encoder gpu" in str(e.value.code) and "\n" not in str(e.value.code)
        monkeypatch.setattr(sys, "argv", base + ["--png_encoder", "gpu", "--png_runs", "--save_format", "jpg"])
        with pytest.raises(SystemExit) as e:
            inf.check_save_format(mod.parse_args())
        assert "--save_format jpg" in str(e.value.code)


def test_encoder_pool_keys_the_mode():
    """pipeline._png_encoder keeps the two modes apart: the same shape and slot in another mode is another entry."""
    import instarevive_amd.png as png
    from instarevive_amd import pipeline

    class Ctx:
        pass
    made = []

    class Fake:
        def __init__(self, ctx, count, h, w, runs=False):
            made.append(runs)
            self.runs = runs
    real, png.PngEncoder = png.PngEncoder, Fake
    try:
        ctx = Ctx()
        a, b = pipeline._png_encoder(ctx, 2, 64, 64), pipeline._png_encoder(ctx, 2, 64, 64, runs=True)
        assert a is not b and a is pipeline._png_encoder(ctx, 2, 64, 64) and b is pipeline._png_encoder(ctx, 2, 64, 64, 0, "sync", True)
        assert made == [False, True]
    finally:
        png.PngEncoder = real
