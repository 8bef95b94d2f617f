"""Host side of the device resampler without a GPU: ir_resample_plan's tables, applied by the numpy statement of the two passes
(tests/support/resample_model.py), must give PIL.Image.resize's bytes - Pillow is the reference and the arithmetic is integer, so every
comparison is exact equality; job_geometry() must give the sizes read_job() produces; the parts of the C ABI that need no device."""
import ctypes as C
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from tests.support import resample_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = {M.BICUBIC: Image.BICUBIC, M.LANCZOS: Image.LANCZOS}

# (filter, (in_h, in_w), (out_h, out_w)); shared with tests/test_resample_gpu.py
CASES = [
    (M.BICUBIC, (33, 90), (188, 512)),
    (M.BICUBIC, (40, 56), (512, 717)),
    (M.BICUBIC, (64, 64), (256, 256)),
    (M.BICUBIC, (1, 1), (4, 4)),
    (M.LANCZOS, (512, 717), (40, 56)),
    (M.LANCZOS, (576, 832), (33, 90)),
    (M.LANCZOS, (50, 50), (50, 71)),    # the vertical pass is skipped
    (M.LANCZOS, (7, 5), (3, 11)),
]
CHECKER_CASES = [(M.BICUBIC, (64, 64), (256, 256)), (M.LANCZOS, (64, 64), (24, 24))]


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def pil_resize(img, out_hw, flt):
    return np.array(Image.fromarray(img).resize((out_hw[1], out_hw[0]), PIL_FILTER[flt]))


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


@pytest.mark.parametrize("flt,in_hw,out_hw", CASES)
def test_plan_tables_give_pillows_bytes_on_noise(flt, in_hw, out_hw):
    _, lib = _library()
    img = noise(*in_hw, seed=in_hw[0])
    p = M.plan(lib, *in_hw, *out_hw, flt)
    assert tuple(p[1:6]) == in_hw + out_hw + (flt,)
    assert (p[6] == 0) == (in_hw[1] == out_hw[1]) and (p[7] == 0) == (in_hw[0] == out_hw[0])   # a skipped pass has no tables
    assert np.array_equal(M.resample(img, p), pil_resize(img, out_hw, flt))


@pytest.mark.parametrize("flt,in_hw,out_hw", CHECKER_CASES)
def test_plan_tables_give_pillows_bytes_where_both_clamps_fire(flt, in_hw, out_hw):
    _, lib = _library()
    img = checkerboard(*in_hw)
    if flt == M.LANCZOS:   # a reduction averages a one-pixel checkerboard to grey: blocks of four keep the edges that overshoot
        img = np.kron(checkerboard(in_hw[0] // 4, in_hw[1] // 4)[:, :, 0], np.ones((4, 4), np.uint8))[:, :, None].repeat(3, 2)
    p = M.plan(lib, *in_hw, *out_hw, flt)
    # the sums before the clamp must really leave 0 .. 255 on both sides, else the case does not test the clamp
    hor, ver = M.tables(p)
    first = img.transpose(1, 0, 2).astype(np.int64)
    raw = np.stack([(1 << 21) + np.tensordot(hor[1][i, :c].astype(np.int64), first[lo:lo + c], axes=(0, 0)) for i, (lo, c) in enumerate(hor[0])]) >> 22
    assert raw.min() < 0 and raw.max() > 255
    assert np.array_equal(M.resample(img, p), pil_resize(img, out_hw, flt))


def test_plan_bytes_agree_with_what_the_plan_accepts():
    _, lib = _library()
    for flt, in_hw, out_hw in CASES + [(M.BICUBIC, (60, 84), (60, 84))]:
        need = int(lib.ir_resample_plan_bytes(*in_hw, *out_hw, flt))
        buf = np.full(need // 4 + 2, -7, np.int32)
        assert lib.ir_resample_plan(*in_hw, *out_hw, flt, C.c_void_p(buf.ctypes.data), need - 1) == -1 and np.all(buf == -7)
        assert lib.ir_resample_plan(*in_hw, *out_hw, flt, C.c_void_p(buf.ctypes.data), need) == 0
        assert buf[12] * 4 == need and np.all(buf[need // 4:] == -7)
    assert lib.ir_resample_plan_bytes(0, 5, 5, 5, 0) == 0 and lib.ir_resample_plan_bytes(5, 5, 5, 0, 1) == 0 and lib.ir_resample_plan_bytes(5, 5, 5, 5, 2) == 0
    buf = np.zeros(64, np.int32)
    assert lib.ir_resample_plan(4, 4, 8, 8, 2, C.c_void_p(buf.ctypes.data), 256) == -1
    assert lib.ir_resample_plan(4, 4, 8, 8, 0, None, 1 << 20) == -1
    assert lib.ir_abi_version() == 3


def test_workspace_and_argument_checks_need_no_gpu():
    L, lib = _library()
    assert L.STAGE_RESAMPLE == 11
    one = lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 1, 512, 2048, 0, 0, 0)
    assert one >= 512 * 2048 * 3 and lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 3, 512, 2048, 0, 0, 0) >= 3 * 512 * 2048 * 3
    assert lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 0, 8, 8, 0, 0, 0) == 0
    fake = C.c_void_p(0x1000)   # never dereferenced: the null context is refused before anything is launched
    assert lib.ir_resample_u8(None, None, fake, 1, 8, 8, 24, fake, 16, 16, 16, 16, 48, fake, fake, 1 << 20) == -1


SIZES = [(64, 64), (56, 40), (90, 33), (512, 512), (640, 512), (520, 600), (300, 700)]   # (w, h)


@pytest.mark.parametrize("tiled,tile_size", [(False, 512), (True, 512), (True, 64)])
@pytest.mark.parametrize("sr_scale", [1, 1.5, 4])
def test_job_geometry_equals_read_job(tmp_path, sr_scale, tiled, tile_size):
    sys.path.insert(0, ROOT)
    import inference as inf
    from instarevive_amd.resample import job_geometry
    (tmp_path / "in").mkdir()
    chained = 0
    for w, h in SIZES:
        path = tmp_path / "in" / f"{w}x{h}.png"
        Image.fromarray(noise(h, w, seed=w + h)).save(path)
        args = Namespace(input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=sr_scale, tiled=tiled, tile_size=tile_size, use_center_crop=False)
        job = inf.read_job(str(path), 0, args)
        geo = job_geometry((w, h), sr_scale, tiled, tile_size)
        assert geo.net_hw + (3,) == job.net_in.shape and tuple(geo.valid_hw) == tuple(job.valid_hw) and geo.lq_size == job.lq.size, (w, h)
        assert geo.lanczos == (None if job.lq.size == (job.valid_hw[1], job.valid_hw[0]) else job.lq.size)
        assert len(geo.chain) == (sr_scale != 1) + (min(job.lq.size) < (tile_size if tiled else 512))
        chained += len(geo.chain) == 2
        # the same file under --resize gpu: decoded only, the geometry attached, batched by the size the device will make
        gjob = inf.read_job(str(path), 0, Namespace(**vars(args), resize_on_gpu=True))
        assert gjob.geo == geo and gjob.raw.shape == (h, w, 3) and gjob.net_in is None and inf.net_shape(gjob) == job.net_in.shape
        assert gjob.save_path == job.save_path and inf.net_shape(job) == job.net_in.shape
        assert inf.png_rect(gjob, Namespace(show_lq=False)) == (job.lq.size[::-1] if geo.lanczos else tuple(job.valid_hw))
        assert inf.png_rect(gjob, Namespace(show_lq=True)) is None
    assert chained > 0 or sr_scale == 1 or (tiled and tile_size == 64 and sr_scale == 4)   # both resizes in one job are covered


def test_two_chained_resizes_through_the_model_equal_read_job(tmp_path):
    """(40, 56) at --sr_scale 1.5, then auto_resize to 512: the plans of job_geometry's chain, applied in turn with a uint8 image between, give
    read_job()'s network input, zero padding included."""
    sys.path.insert(0, ROOT)
    import inference as inf
    from instarevive_amd.resample import job_geometry
    _, lib = _library()
    (tmp_path / "in").mkdir()
    img = noise(40, 56, seed=11)
    Image.fromarray(img).save(tmp_path / "in" / "a.png")
    job = inf.read_job(str(tmp_path / "in" / "a.png"), 0, Namespace(input=str(tmp_path / "in"), output="o", sr_scale=1.5, tiled=False, tile_size=512, use_center_crop=False))
    geo = job_geometry((56, 40), 1.5, False, 512)
    assert len(geo.chain) == 2
    for tw, th in geo.chain:
        img = M.resample(img, M.plan(lib, img.shape[0], img.shape[1], th, tw, M.BICUBIC))
    want = job.net_in
    assert np.array_equal(img, want[:img.shape[0], :img.shape[1]]) and not want[img.shape[0]:].any() and not want[:, img.shape[1]:].any()


def test_parser_default_is_the_host_resize(monkeypatch):
    sys.path.insert(0, ROOT)
    import inference as inf
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o"])
    assert inf.parse_args().resize == "host"
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--resize", "gpu"])
    assert inf.parse_args().resize == "gpu"
    monkeypatch.setattr(sys, "argv", ["inference.py", "--ckpt", "c", "--input", "i", "--output", "o", "--resize", "fpga"])
    with pytest.raises(SystemExit):
        inf.parse_args()
