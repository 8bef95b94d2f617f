"""The centre crop's device route without a GPU: ir_resample_plan's BOX tables through the numpy statement of the two 8-bit passes must give
PIL.Image.resize(..., BOX)'s bytes; crop_geometry() and the model of the whole chain (every plan in turn, the last one applied to the window's
rows and columns alone, as ir_resample_u8_window does) must give decode_job()'s --sr_scale resize + center_crop_arr in sizes, offsets and
bytes; the flag checks of both command lines; the parts of the C ABI that need no device. Integer arithmetic throughout: exact equality."""
import ctypes as C
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from tests.support import resample_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = 4   # Pillow's own number
S = 64

# ((in_h, in_w), (out_h, out_w)); shared with tests/test_center_crop_gpu.py
BOX_CASES = [
    ((48, 64), (24, 32)),      # exact halves
    ((47, 65), (23, 32)),      # floor halves: three-tap windows
    ((3, 1001), (1, 500)),
    ((37, 100), (5, 7)),
    ((40, 90), (40, 45)),      # one axis unchanged: the vertical pass is skipped
    ((90, 40), (45, 40)),      # the horizontal pass is skipped
]

# ((w, h) of the file, sr_scale, image_size); shared with tests/test_center_crop_gpu.py. At image_size 64 the scaled edge e * 64 / m with the short edge
# m < 128 is never an exact .5 (that needs 128 | m * odd), so the case that tells Python's round from a round-half-up is at image_size 48:
# 35 * (48 / 32) = 52.5 -> 52.
FILES = [
    ((64, 64), 1, S),        # nothing to do
    ((300, 128), 1, S),      # short edge exactly 2 S: one halving, then an identity resize
    ((301, 127), 1, S),      # just below: no halving
    ((257, 131), 1, S),
    ((515, 131), 1, S),
    ((131, 515), 1, S),
    ((40, 56), 1, S),        # enlarged
    ((1030, 259), 1, S),     # two halvings, odd sizes
    ((56, 40), 1.5, S),
    ((32, 35), 1, 48),       # 52.5: round half to even
]


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _library():
    from instarevive_amd import _lib as L
    return L, L.load_library()


def host_crop(img: np.ndarray, sr_scale: float, image_size: int) -> np.ndarray:
    """decode_job()'s PIL code under --use_center_crop: the --sr_scale bicubic, then center_crop_arr."""
    import math
    from instarevive_amd.utils import center_crop_arr
    lq = Image.fromarray(img)
    if sr_scale != 1:
        lq = lq.resize(tuple(math.ceil(edge * sr_scale) for edge in lq.size), Image.BICUBIC)
    return np.array(center_crop_arr(lq, image_size))


def window_model(img: np.ndarray, p: np.ndarray, y0: int, x0: int, win_h: int, win_w: int) -> np.ndarray:
    """ir_resample_u8_window by the plan p: the horizontal pass of columns x0 .. x0 + win_w (of every row: the rows the vertical taps do not
    reach change nothing), the vertical pass of rows y0 .. y0 + win_h; a skipped pass cuts."""
    hor, ver = M.tables(p)
    if hor is not None:
        img = M.one_pass(img.transpose(1, 0, 2), hor[0][x0:x0 + win_w], hor[1][x0:x0 + win_w]).transpose(1, 0, 2)
    else:
        img = img[:, x0:x0 + win_w]
    if ver is not None:
        img = M.one_pass(img, ver[0][y0:y0 + win_h], ver[1][y0:y0 + win_h])
    else:
        img = img[y0:y0 + win_h]
    return np.ascontiguousarray(img)


def chain_model(lib, img: np.ndarray, geo) -> np.ndarray:
    """The crop of a crop_geometry() by the plans: every step but the last in full (a step of equal size copies), the last as a window."""
    flts = geo.filters
    for (tw, th), flt in zip(geo.chain[:-1], flts[:-1]):
        if img.shape[:2] != (th, tw):
            img = M.resample(img, M.plan(lib, img.shape[0], img.shape[1], th, tw, flt))
    tw, th = geo.chain[-1]
    return window_model(img, M.plan(lib, img.shape[0], img.shape[1], th, tw, flts[-1]), *geo.crop, *geo.valid_hw)


# ---------------------------------------------------------------------------------------------------------------- the BOX plan
@pytest.mark.parametrize("in_hw,out_hw", BOX_CASES)
def test_box_plan_tables_give_pillows_bytes(in_hw, out_hw):
    _, lib = _library()
    img = noise(*in_hw, seed=in_hw[1])
    p = M.plan(lib, *in_hw, *out_hw, BOX)
    assert tuple(p[1:6]) == in_hw + out_hw + (BOX,)
    assert (p[6] == 0) == (in_hw[1] == out_hw[1]) and (p[7] == 0) == (in_hw[0] == out_hw[0])
    want = np.array(Image.fromarray(img).resize((out_hw[1], out_hw[0]), Image.BOX))
    assert np.array_equal(M.resample(img, p), want)


def test_filter_ids_two_and_three_still_have_no_plan():
    L, lib = _library()
    assert L.RESAMPLE_BOX == BOX == Image.BOX
    buf = np.zeros(1024, np.int32)
    for flt in (2, 3, 5, -1):
        assert lib.ir_resample_plan_bytes(8, 8, 4, 4, flt) == 0
        assert lib.ir_resample_plan(8, 8, 4, 4, flt, C.c_void_p(buf.ctypes.data), 4096) == -1
    assert lib.ir_resample_plan_bytes(8, 8, 4, 4, BOX) > 0


# ---------------------------------------------------------------------------------------------------------------- geometry and pixels
@pytest.mark.parametrize("size,sr_scale,image_size", FILES)
def test_crop_geometry_and_the_chain_model_equal_the_host_crop(size, sr_scale, image_size):
    import math
    from instarevive_amd.resample import BICUBIC, BOX as RBOX, ResizeJob, check_records, crop_geometry
    _, lib = _library()
    w, h = size
    img = noise(h, w, seed=w + h)
    geo = crop_geometry(size, sr_scale, image_size)
    # the sizes PIL goes through
    lq = Image.fromarray(img)
    sizes = []
    if sr_scale != 1:
        lq = lq.resize(tuple(math.ceil(edge * sr_scale) for edge in lq.size), Image.BICUBIC)
        sizes.append(lq.size)
    while min(lq.size) >= 2 * image_size:
        lq = lq.resize(tuple(edge // 2 for edge in lq.size), Image.BOX)
        sizes.append(lq.size)
    halvings = len(sizes) - (sr_scale != 1)
    lq = lq.resize(tuple(round(edge * (image_size / min(lq.size))) for edge in lq.size), Image.BICUBIC)
    sizes.append(lq.size)
    assert list(geo.chain) == sizes
    assert list(geo.filters) == [BICUBIC] * (sr_scale != 1) + [RBOX] * halvings + [BICUBIC]
    assert geo.crop == ((lq.size[1] - image_size) // 2, (lq.size[0] - image_size) // 2)
    assert geo.valid_hw == geo.net_hw == (image_size, image_size) and geo.lanczos is None
    want = host_crop(img, sr_scale, image_size)
    assert want.shape == (image_size, image_size, 3)
    assert np.array_equal(chain_model(lib, img, geo), want)
    assert check_records([ResizeJob(img, geo)]) == (1, image_size, image_size)


def test_the_file_list_covers_what_it_names():
    from instarevive_amd.resample import BOX as RBOX, crop_geometry
    geos = [crop_geometry(*f) for f in FILES]
    assert geos[0].chain == ((64, 64),) and geos[0].crop == (0, 0)
    assert geos[1].chain == ((150, 64), (150, 64)) and geos[1].filters.count(RBOX) == 1
    assert geos[2].filters.count(RBOX) == 0
    assert geos[7].filters.count(RBOX) == 2 and geos[7].chain[0] == (515, 129)
    assert len(geos[8].chain) == 2 and geos[8].chain[0] == (84, 60)
    assert geos[9].chain == ((48, 52),)   # 52.5 -> 52, not 53
    assert any(g.crop[1] % 4 for g in geos) and any(g.crop[0] for g in geos)   # windows off the dword grid, and off the top


def test_old_form_geometry_means_what_it_meant():
    """Geometry(chain, valid_hw, net_hw, lq_size, lanczos): no filters, no crop, and _steps / check_records / chain_ws_bytes as for job_geometry."""
    from instarevive_amd import resample as R
    for size, sr in (((56, 40), 1.5), ((64, 64), 1), ((300, 700), 1), ((90, 33), 4)):
        geo = R.job_geometry(size, sr, False, 512)
        old = R.Geometry(geo.chain, geo.valid_hw, geo.net_hw, geo.lq_size, geo.lanczos)
        assert old == geo and old.crop is None and old.filters == () and len(old) == 7 and old[:5] == tuple(geo)[:5]
        rec = R.ResizeJob(noise(size[1], size[0]), old)
        sizes = [(size[1], size[0])] + [(th, tw) for tw, th in geo.chain]
        want = [a + b for a, b in zip(sizes[:-1], sizes[1:])] or [sizes[0] + sizes[0]]
        assert R._steps(rec) == want
        assert R.check_records([rec]) == (1,) + tuple(geo.net_hw)
        assert R.chain_ws_bytes([rec]) == max([R.ws_bytes(1, *s) for s in want] + ([R.ws_bytes(1, *geo.valid_hw, geo.lanczos[1], geo.lanczos[0])] if geo.lanczos else []))
    with pytest.raises(ValueError, match="does not belong"):
        R.check_records([R.ResizeJob(noise(40, 56), R.Geometry((), (41, 56), (64, 64), (56, 40), None))])


def test_crop_records_are_checked_and_sized():
    from instarevive_amd import resample as R
    img = noise(259, 1030)
    geo = R.crop_geometry((1030, 259), 1, S)
    rec = R.ResizeJob(img, geo)
    assert [s[4] for s in R._crop_steps(rec)] == [R.BOX, R.BOX, R.BICUBIC] and R._steps(rec) == [s[:4] for s in R._crop_steps(rec)]
    # nothing to do / an identity resize behind a halving: the equal-sized steps are skipped but for the last, which is the window call
    assert R._steps(R.ResizeJob(noise(64, 64), R.crop_geometry((64, 64), 1, S))) == [(64, 64, 64, 64)]
    assert R._steps(R.ResizeJob(noise(128, 300), R.crop_geometry((300, 128), 1, S))) == [(128, 300, 64, 150), (64, 150, 64, 150)]
    lib = _library()[1]
    rec = R.ResizeJob(noise(131, 515), R.crop_geometry((515, 131), 1, S))   # 257 x 65 -> 253 x 64: both passes run in the window call
    ih, iw, oh, ow = R._steps(rec)[-1]
    assert (ih, iw, oh, ow) == (65, 257, 64, 253)
    assert R.window_ws_bytes(1, ih, iw, oh, ow, S) == lib.ir_workspace_bytes(None, 11, 1, ih, S, 0, 0, 0) > 0
    assert R.chain_ws_bytes([rec]) >= max(R.ws_bytes(1, *s) for s in R._steps(rec)[:-1])
    with pytest.raises(ValueError, match="window"):
        R.check_records([R.ResizeJob(noise(259, 1030), geo._replace(crop=(0, geo.chain[-1][0] - S + 1)))])
    with pytest.raises(ValueError, match="one network input size"):
        R.check_records([R.ResizeJob(img, geo), R.ResizeJob(noise(35, 32), R.crop_geometry((32, 35), 1, 48))])


# ---------------------------------------------------------------------------------------------------------------- flags
def _ns(**kw):
    base = dict(use_center_crop=False, center_crop="host", tiled=False, show_lq=False, shard_tiles=False, resize="host", jpeg_decoder="host")
    base.update(kw)
    return Namespace(**base)


def test_check_center_crop_at_function_level(capsys):
    sys.path.insert(0, ROOT)
    import inference as inf
    from instarevive_amd import degrade as D
    inf.check_center_crop(_ns())                         # host: nothing happens
    inf.check_center_crop(Namespace(resize="host"))      # a Namespace without the attribute is the host crop
    with pytest.raises(SystemExit) as e:
        inf.check_center_crop(_ns(center_crop="gpu"))
    assert "--center_crop gpu" in str(e.value) and "--use_center_crop" in str(e.value) and "\n" not in str(e.value)
    for flag in ("tiled", "show_lq", "shard_tiles"):
        with pytest.raises(SystemExit) as e:
            inf.check_center_crop(_ns(center_crop="gpu", use_center_crop=True, **{flag: True}))
        assert "--center_crop gpu" in str(e.value) and f"--{flag}" in str(e.value) and "\n" not in str(e.value)
    args = _ns(center_crop="gpu", use_center_crop=True, jpeg_decoder="gpu")
    inf.check_center_crop(args)
    assert args.resize == "gpu" and "switching --resize gpu on" in capsys.readouterr().out
    inf.check_jpeg_decoder(args)                         # accepted next to --jpeg_decoder gpu ...
    D.check_flags(args)                                  # ... and next to --degrade
    # the host crop keeps both refusals, with or without the new attribute
    with pytest.raises(SystemExit, match="--use_center_crop keeps on the host"):
        inf.check_jpeg_decoder(_ns(use_center_crop=True, jpeg_decoder="gpu"))
    with pytest.raises(D.DegradeError, match="cannot be combined with --use_center_crop"):
        D.check_flags(_ns(use_center_crop=True))
    with pytest.raises(D.DegradeError, match="cannot be combined with --use_center_crop"):
        D.check_flags(Namespace(use_center_crop=True, show_lq=False, shard_tiles=False))
    with pytest.raises(D.DegradeError, match="--show_lq"):
        D.check_flags(_ns(center_crop="gpu", use_center_crop=True, show_lq=True))


@pytest.mark.parametrize("sr_scale", [1, 1.5])
def test_ground_truth_of_a_degraded_crop_is_cropped_on_the_host(tmp_path, sr_scale):
    """--degrade with --center_crop gpu: what is degraded is the 512 x 512 crop, so attach_gt() crops the ground truth by the same rule - the
    decoded input itself without --gt, a full-size file of a --gt folder otherwise; a ground truth that is 512 x 512 already is taken as it is."""
    from types import SimpleNamespace
    sys.path.insert(0, ROOT)
    import inference as inf
    from instarevive_amd import degrade as D
    (tmp_path / "in").mkdir()
    (tmp_path / "gt").mkdir()
    img, other = noise(520, 700, seed=1), noise(520, 700, seed=2)
    Image.fromarray(img).save(tmp_path / "in" / "a.png")
    Image.fromarray(other).save(tmp_path / "gt" / "a.png")
    args = Namespace(input=str(tmp_path / "in"), output=str(tmp_path / "out"), sr_scale=sr_scale, tiled=False, tile_size=512, use_center_crop=True,
                     center_crop="gpu", resize_on_gpu=True, show_lq=False, degrade_recipe=D.load_recipe("lq"), degrade_seed=3)
    src = str(tmp_path / "in" / "a.png")
    for folder, pixels in (("in", img), ("gt", other)):
        args.gt_lookup = SimpleNamespace(path=lambda f, folder=folder: str(tmp_path / folder / "a.png"))
        job = inf.read_job(src, 0, args)
        assert job.geo.crop is not None and job.raw.shape == (520, 700, 3) and inf.png_rect(job, args) == (512, 512)
        assert (job.deg.lh, job.deg.lw) <= (512, 512) and job.deg.noise.shape[:2] == (job.deg.lh, job.deg.lw)   # drawn for the crop
        assert job.gt.shape == (512, 512, 3) and np.array_equal(job.gt, host_crop(pixels, sr_scale, 512))
    ready = noise(512, 512, seed=3)
    Image.fromarray(ready).save(tmp_path / "gt" / "a.png")
    assert np.array_equal(inf.read_job(src, 0, args).gt, ready)
    # without --degrade nothing is cropped: a ground truth of another size is refused as before
    from instarevive_amd.metrics import MetricsError
    args.degrade_recipe = None
    Image.fromarray(other).save(tmp_path / "gt" / "a.png")
    with pytest.raises(MetricsError, match="512 x 512"):
        inf.read_job(src, 0, args)


def test_parser_default_is_the_host_crop(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_batch as ev
    import inference as inf
    for mod in (inf, ev):
        monkeypatch.setattr(sys, "argv", ["x.py", "--ckpt", "c", "--input", "i", "--output", "o"])
        assert mod.parse_args().center_crop == "host"
        monkeypatch.setattr(sys, "argv", ["x.py", "--ckpt", "c", "--input", "i", "--output", "o", "--center_crop", "gpu"])
        assert mod.parse_args().center_crop == "gpu"
        monkeypatch.setattr(sys, "argv", ["x.py", "--ckpt", "c", "--input", "i", "--output", "o", "--center_crop", "fpga"])
        with pytest.raises(SystemExit):
            mod.parse_args()


def _cli(script, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), "--ckpt", "x", "--input", "in", "--output", "out", *flags],
                          capture_output=True, text=True, timeout=300, cwd=ROOT)


def _one_line(r):
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert r.returncode != 0 and len(lines) == 1, r.stderr[-1500:]
    return lines[0]


@pytest.mark.parametrize("flags,named", [
    ((), "--use_center_crop"),
    (("--use_center_crop", "--tiled"), "--tiled"),
    (("--use_center_crop", "--show_lq"), "--show_lq"),
    (("--use_center_crop", "--shard_tiles"), "--shard_tiles"),
])
def test_cli_refuses_center_crop_gpu_in_one_line(flags, named):
    line = _one_line(_cli("inference.py", "--center_crop", "gpu", *flags))
    assert "--center_crop gpu" in line and named in line


@pytest.mark.parametrize("extra", [("--jpeg_decoder", "gpu"), ("--degrade",)])
def test_cli_accepts_the_crop_next_to_the_device_routes(extra):
    """Past every argument check: the run ends at the device check (no GPU here) or, with one, at the checkpoint that does not exist - not at a
    refusal that names the flags."""
    r = _cli("inference.py", "--use_center_crop", "--center_crop", "gpu", "--device", "cpu", *extra)
    line = _one_line(r)
    assert "device 'cpu' requested" in line and "switching --resize gpu on" in r.stdout
    # the host crop is refused as before, in one line that may carry the hint
    line = _one_line(_cli("inference.py", "--use_center_crop", "--device", "cpu", *extra))
    assert "--use_center_crop" in line and "--center_crop gpu" in line and "device 'cpu'" not in line


def test_eval_batch_takes_the_device_decoder_with_the_device_crop():
    line = _one_line(_cli("eval_batch.py", "--jpeg_decoder", "gpu"))
    assert "--jpeg_decoder gpu" in line and "device 'cpu'" not in line
    line = _one_line(_cli("eval_batch.py", "--jpeg_decoder", "gpu", "--center_crop", "gpu", "--device", "cpu"))
    assert "device 'cpu' requested" in line


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_window_call_is_exported_and_refuses_without_a_device():
    L, lib = _library()
    assert "ir_resample_u8_window" in L.SYMBOLS and hasattr(lib, "ir_resample_u8_window") and lib.ir_abi_version() == 3
    with open(os.path.join(ROOT, "include", "instarevive_hip.h")) as f:
        header = f.read()
    assert "int ir_resample_u8_window(" in header and "IR_RESAMPLE_BOX = 4" in header
    fake = C.c_void_p(0x1000)   # never dereferenced: every refusal comes before anything is launched

    def call(i=fake, o=fake, p=fake):
        return lib.ir_resample_u8_window(None, None, i, 1, 8, 8, 24, o, 16, 16, 2, 3, 8, 8, 8, 8, 24, p, fake, 1 << 20)

    # no context exists without a device, so only the null checks can be reached here; the refusals of windows, full sizes and pitches are
    # varied one by one in tests/test_center_crop_gpu.py
    assert call() == -1 and call(i=None) == -1 and call(o=None) == -1 and call(p=None) == -1
