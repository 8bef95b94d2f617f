"""The centre crop on the device: ir_resample_u8 with BOX plans, ir_resample_u8_window, crop geometries through resample.ResizeSlot (alone,
from a JPEG the device decodes, and ahead of ir_degrade) and --center_crop gpu of both command lines. Pillow / center_crop_arr is the
reference and the arithmetic is integer: every comparison is exact equality."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import resample_model as M
from tests.test_center_crop_cpu import BOX, BOX_CASES, FILES, S, host_crop, noise

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


# ---------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("in_hw,out_hw", BOX_CASES)
def test_box_plans_on_the_device_equal_pillow(in_hw, out_hw):
    from tests.test_resample_gpu import _resample
    imgs = np.stack([noise(*in_hw, seed=s) for s in (3, 4)])
    rc, out, tail = _resample(imgs, out_hw, BOX)
    assert rc == 0 and np.all(tail == CANARY)
    for i in range(2):
        want = np.array(Image.fromarray(imgs[i]).resize((out_hw[1], out_hw[0]), Image.BOX))
        assert np.array_equal(out[i].reshape(out_hw + (3,)), want)


def _window(imgs, out_hw, flt, y0, x0, win_h, win_w, full_hw=None, extra_pitch=0, head=64, slack=256):
    """ir_resample_u8_window on imgs [n][in_h][in_w][3] into a canary-filled buffer: `head` bytes, then [n][full_h][out_pitch], then `slack`
    bytes. -> (rc, head, the destination, slack). The workspace is given 16 bytes more than the call is told of, which must stay untouched."""
    ctx = _ctx()
    n, in_h, in_w, _ = imgs.shape
    full_h, full_w = full_hw or (win_h, win_w)
    out_pitch = 3 * full_w + extra_pitch
    d_in = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    body = n * full_h * out_pitch
    d_out = torch.full((head + body + slack,), CANARY, dtype=torch.uint8, device="cuda")
    plan = torch.from_numpy(M.plan(ctx.lib, in_h, in_w, *out_hw, flt)).cuda()
    need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, n, in_h, win_w, 0, 0, 0))
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.ir_resample_u8_window(ctx.h, ctx.stream(), L.ptr(d_in), n, in_h, in_w, 3 * in_w, C.c_void_p(d_out.data_ptr() + head), out_hw[0], out_hw[1],
                                       y0, x0, win_h, win_w, full_h, full_w, out_pitch, L.ptr(plan), L.ptr(ws), need)
    torch.cuda.synchronize()
    assert bool((ws[need:] == CANARY).all())
    out = d_out.cpu().numpy()
    return rc, out[:head], out[head:head + body].reshape(n, full_h, out_pitch), out[head + body:]


_FULL = {}


def _full(key, in_hw, out_hw, flt):
    """The whole ir_resample_u8 result of a case's two images, computed once and shared (read-only)."""
    if key not in _FULL:
        from tests.test_resample_gpu import _resample
        imgs = np.stack([noise(*in_hw, seed=s) for s in (11, 12)])
        rc, out, _ = _resample(imgs, out_hw, flt)
        assert rc == 0
        _FULL[key] = (imgs, out.reshape((2,) + out_hw + (3,)))
    return _FULL[key]


# (key, filter, (in_h, in_w), (out_h, out_w)): both passes; then only the horizontal, only the vertical, neither
WINDOW_CASES = {
    "bicubic": (M.BICUBIC, (127, 90), (90, 64)),
    "box": (BOX, (257, 131), (128, 65)),
    "hor": (M.BICUBIC, (70, 90), (70, 64)),
    "ver": (BOX, (140, 65), (70, 65)),
    "copy": (M.BICUBIC, (70, 65), (70, 65)),
    # the same two with a source pitch that is a multiple of 4: the dword loads run where 3 * x0 is one too, the byte fallback elsewhere
    "ver4": (BOX, (140, 64), (70, 64)),
    "copy4": (M.BICUBIC, (70, 64), (70, 64)),
}


def _windows(out_h, out_w):
    """(y0, x0, win_h, win_w, full_hw, extra_pitch): at the origin, the whole result, odd x0, x0 a multiple of 4 (the left edge on a dword), touching the right and bottom edges, one pixel wide,
    one pixel, padded to a larger full size with a pitch beyond it (an odd one too: the byte-store path)."""
    return [
        (0, 0, out_h // 2, out_w // 2, None, 0),
        (0, 0, out_h, out_w, None, 0),
        (3, 5, 20, 21, None, 0),
        (2, 8, 20, 21, None, 0),
        (out_h - 17, out_w - 13, 17, 13, None, 0),
        (7, 9, 30, 1, None, 0),
        (out_h - 1, out_w - 1, 1, 1, None, 0),
        (5, 7, 33, 22, (64, 40), 8),
        (6, 1, 33, 22, (35, 22), 5),
    ]


@pytest.mark.parametrize("key", list(WINDOW_CASES))
def test_window_equals_the_cut_of_the_full_call(key):
    flt, in_hw, out_hw = WINDOW_CASES[key]
    imgs, full = _full(key, in_hw, out_hw, flt)
    for y0, x0, wh, ww, full_hw, extra in _windows(*out_hw):
        rc, head, out, tail = _window(imgs, out_hw, flt, y0, x0, wh, ww, full_hw, extra)
        case = (key, y0, x0, wh, ww, full_hw, extra)
        assert rc == 0 and np.all(head == CANARY) and np.all(tail == CANARY), case
        fh, fw = full_hw or (wh, ww)
        for i in range(2):
            assert np.array_equal(out[i, :wh, :3 * ww].reshape(wh, ww, 3), full[i, y0:y0 + wh, x0:x0 + ww]), case
            assert not out[i, wh:, :3 * fw].any() and not out[i, :, 3 * ww:3 * fw].any(), case
            assert np.all(out[i, :, 3 * fw:] == CANARY), case


def test_window_refusals_return_minus_one_and_write_nothing():
    ctx = _ctx()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((16 * 16 * 3,), CANARY, dtype=torch.uint8, device="cuda")
    plan = torch.from_numpy(M.plan(ctx.lib, 8, 8, 16, 16, M.BICUBIC)).cuda()
    need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 1, 8, 6, 0, 0, 0))
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")

    def call(i=img, n=1, in_h=8, in_w=8, in_pitch=24, o=out, out_h=16, out_w=16, y0=2, x0=3, win_h=5, win_w=6, full_h=8, full_w=8, out_pitch=24, p=plan,
             w=ws.data_ptr(), wb=need):
        return ctx.lib.ir_resample_u8_window(ctx.h, ctx.stream(), L.ptr(i), n, in_h, in_w, in_pitch, L.ptr(o), out_h, out_w, y0, x0, win_h, win_w, full_h,
                                             full_w, out_pitch, L.ptr(p), C.c_void_p(w), wb)

    refused = {
        "null in": call(i=None), "null out": call(o=None), "null plan": call(p=None), "null workspace": call(w=None),
        "n": call(n=0), "in_h": call(in_h=0), "in_w": call(in_w=0), "out_h": call(out_h=0), "out_w": call(out_w=0), "in_pitch": call(in_pitch=23),
        "window below": call(y0=12), "window right": call(x0=11), "negative y0": call(y0=-1), "negative x0": call(x0=-1),
        "empty window": call(win_h=0), "empty window w": call(win_w=0),
        "full_h < win_h": call(full_h=4), "full_w < win_w": call(full_w=5), "out_pitch < 3 full_w": call(out_pitch=23),
        "short workspace": call(wb=need - 1), "unaligned workspace": call(w=ws.data_ptr() + 1),
    }
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in refused.values()), {k: v for k, v in refused.items() if v != -1}
    assert bool((out == CANARY).all()) and b"ir_resample_u8_window" in ctx.lib.ir_last_error(ctx.h)
    assert call(y0=11, x0=10) == 0   # the window that touches both edges is inside
    torch.cuda.synchronize()
    assert not bool((out[:8 * 24] == CANARY).all()) and bool((out[8 * 24:] == CANARY).all())


# ---------------------------------------------------------------------------------------------------------------- ResizeSlot
def _slot_run(records, image_size, degrade=None):
    """fill / upload / decode / [degrade] / to_network of one batch -> (the network input [n][S][S][3], the downloaded LQ images or None)."""
    from instarevive_amd.resample import ResizeSlot, chain_ws_bytes, check_records, decode_ws_bytes
    ctx = _ctx()
    assert check_records(records) == (len(records), image_size, image_size)
    rs = ResizeSlot(ctx)
    rs.fill(records, degrade)
    rs.upload()
    ctx.workspace(max(chain_ws_bytes(records), decode_ws_bytes(records), 1))
    rs.decode(records)
    if degrade is not None:
        rs.degrade(records)
        rs.download_lq()
    d_in = torch.full((len(records), image_size, image_size, 3), CANARY, dtype=torch.uint8, device="cuda")
    rs.to_network(records, d_in)
    rs.download_info()
    torch.cuda.synchronize()
    rs.check_info(records)
    return d_in.cpu().numpy(), rs.host_lq(records) if degrade is not None else None


def test_crop_geometries_through_the_slot_equal_center_crop_arr():
    """Every file of the list in one batch per image size (the --sr_scale case included): chains of one to three calls, windows off the dword grid."""
    from instarevive_amd.resample import ResizeJob, crop_geometry
    for size in (S, 48):
        files = [f for f in FILES if f[2] == size]
        imgs = [noise(h, w, seed=w * h) for (w, h), _, _ in files]
        records = [ResizeJob(img, crop_geometry(wh, sr, size)) for img, (wh, sr, _) in zip(imgs, files)]
        got, _ = _slot_run(records, size)
        for k, (img, (wh, sr, _)) in enumerate(zip(imgs, files)):
            assert np.array_equal(got[k], host_crop(img, sr, size)), (wh, sr, size)


def test_a_jpeg_decoded_on_the_device_is_cropped_like_pillows_pixels():
    import io
    from instarevive_amd.jpeg_decode import JpegSource
    from instarevive_amd.resample import ResizeJob, crop_geometry
    from instarevive_amd.utils import center_crop_arr
    from tests.test_jpeg_cpu import content
    buf = io.BytesIO()
    Image.fromarray(content(257, 131)[1]).save(buf, format="JPEG", quality=90, subsampling="4:2:0")   # w x h = 131 x 257
    src, why = JpegSource.open(buf.getvalue())
    assert src is not None, why
    assert tuple(src.shape[:2]) == (257, 131)
    other = noise(131, 515, seed=2)   # a decoded file next to it in the batch
    records = [ResizeJob(src, crop_geometry((131, 257), 1, S)), ResizeJob(other, crop_geometry((515, 131), 1, S))]
    got, _ = _slot_run(records, S)
    assert np.array_equal(got[0], center_crop_arr(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"), S))
    assert np.array_equal(got[1], host_crop(other, 1, S))


def test_the_crop_is_what_is_degraded():
    """degrade=: the crop is made first, ir_degrade / ir_degrade_chain read it, the parameters are those of an image_size x image_size file. The
    downloaded LQ image - and the network input - is the numpy model applied to the host-made crop. `lq` at 64; `realesrgan` at 64 as well
    (its chains need 44 pixels on the short side)."""
    from instarevive_amd import degrade as D
    from instarevive_amd.resample import ResizeJob, crop_geometry
    from tools import degrade_folder as DM
    sizes = [(515, 131), (300, 128), (40, 56)]
    imgs = [noise(h, w, seed=w) for w, h in sizes]
    records = [ResizeJob(img, crop_geometry(wh, 1, S)) for img, wh in zip(imgs, sizes)]
    crops = [host_crop(img, 1, S) for img in imgs]
    ps = [D.draw(D.load_recipe("lq"), f"f{i}.png", S, S, 231) for i in range(3)]
    got, lqs = _slot_run(records, S, ps)
    for k, (crop, p) in enumerate(zip(crops, ps)):
        want = DM.degrade_model(crop, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)
        assert lqs[k].shape == (S, S, 3) and np.array_equal(lqs[k], want) and np.array_equal(got[k], want), sizes[k]
    from tests.test_degrade_chain_gpu import _drawable
    chains = [_drawable(D.load_recipe("realesrgan"), S, S, 7 + i)[1] for i in range(3)]
    assert all(isinstance(p, D.ChainParams) for p in chains)
    got, lqs = _slot_run(records, S, chains)
    for k, (crop, p) in enumerate(zip(crops, chains)):
        want = DM.degrade_chain_model(crop, p.ops)
        assert np.array_equal(lqs[k], want) and np.array_equal(got[k], want), sizes[k]


def test_a_batch_may_mix_crops_and_plain_files_under_degrade():
    """A large file that is cropped in front of a plain file and one that is enlarged, all to one 64 x 64 network input, with degrade=: the LQ
    images lie at offsets of their own (the crop is far smaller than its file), and every record's network input is made from ITS LQ image."""
    from instarevive_amd import degrade as D
    from instarevive_amd.resample import ResizeJob, crop_geometry, job_geometry
    from tools import degrade_folder as DM
    big, plain, small = noise(131, 515, seed=1), noise(64, 64, seed=2), noise(48, 48, seed=3)
    records = [ResizeJob(big, crop_geometry((515, 131), 1, S)), ResizeJob(plain, job_geometry((64, 64), 1, True, 64)),
               ResizeJob(small, job_geometry((48, 48), 1, True, 64))]
    assert [r.geo.net_hw for r in records] == [(S, S)] * 3 and len(records[2].geo.chain) == 1
    gts = [host_crop(big, 1, S), plain, small]
    ps = [D.draw(D.load_recipe("lq"), f"m{i}.png", g.shape[0], g.shape[1], 231) for i, g in enumerate(gts)]
    got, lqs = _slot_run(records, S, ps)
    for k, (g, p) in enumerate(zip(gts, ps)):
        want = DM.degrade_model(g, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)
        assert np.array_equal(lqs[k], want), k
        if k == 2:   # the enlarged file: the bicubic of its LQ image
            want = np.array(Image.fromarray(want).resize((64, 64), Image.BICUBIC))
        assert np.array_equal(got[k], want), k


def test_process_takes_crop_jobs_and_returns_the_run_on_the_host_crop():
    """process(resize=[ResizeJob(raw, crop_geometry(...))]) on the reduced models: the image_size x image_size prediction of a run that is fed the
    host-made crop, scored like it."""
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, crop_geometry, job_geometry
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    sizes = [(257, 131), (1030, 259)]
    imgs = [noise(h, w, seed=h) for w, h in sizes]
    crops = [host_crop(img, 1, S) for img in imgs]
    gts = [noise(S, S, seed=5), noise(S, S, seed=6)]
    got = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(i, crop_geometry(wh, 1, S)) for i, wh in zip(imgs, sizes)], gt=gts, **kw)
    plain = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(c, job_geometry((S, S), 1, True, 64)) for c in crops], gt=gts, **kw)
    for k in range(2):
        assert got[0][k].shape == (S, S, 3) and np.array_equal(got[0][k], plain[0][k]) and np.array_equal(got[1][k], plain[1][k])
    assert got[2] == plain[2]


# ---------------------------------------------------------------------------------------------------------------- command lines
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _models(d):
    return ["--ckpt", str(d / "weights" / "dit.ckpt"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae",
            str(d / "vae"), "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth")]


def _photo_like(h, w, seed):
    """Smooth content with some texture: what a JPEG codes without ringing over the whole range."""
    from tests.test_degrade_chain_gpu import _image
    return _image(h, w, seed)


def _same_trees(a, b, count):
    assert sorted(a) == sorted(b) and len(a) == count, (sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def test_cli_center_crop_gpu_writes_the_host_pixels_and_scores(tmp_path):
    """inference.py --use_center_crop --gt on a 700 x 520 PNG and a 1100 x 1300 JPEG (one halving): --center_crop gpu saves the pixels and the
    metrics.csv of --center_crop host (the route next to --jpeg_decoder gpu runs in the eval_batch.py case)."""
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _decode_tree
    d = tmp_path
    _write_artifacts(d)
    for f in (d / "in").glob("**/*") if (d / "in").exists() else ():
        if f.is_file():
            f.unlink()
    os.makedirs(d / "in" / "sub", exist_ok=True)
    os.makedirs(d / "gt" / "sub", exist_ok=True)
    Image.fromarray(_photo_like(520, 700, 1)).save(d / "in" / "a.png")
    Image.fromarray(_photo_like(1300, 1100, 2)).save(d / "in" / "sub" / "b.jpg", quality=90)
    Image.fromarray(_photo_like(512, 512, 3)).save(d / "gt" / "a.png")
    Image.fromarray(_photo_like(512, 512, 4)).save(d / "gt" / "sub" / "b.png")
    base = [sys.executable, os.path.join(ROOT, "inference.py"), "--input", str(d / "in"), *_models(d), "--batch_size", "2", "--workers", "2", "--use_center_crop",
            "--gt", str(d / "gt")]
    _run(base + ["--output", str(d / "host"), "--metrics_out", str(d / "host.csv"), "--center_crop", "host"])
    out = _run(base + ["--output", str(d / "gpu"), "--metrics_out", str(d / "gpu.csv"), "--center_crop", "gpu"])
    assert "switching --resize gpu on" in out
    host, gpu = _decode_tree(d / "host"), _decode_tree(d / "gpu")
    _same_trees(host, gpu, 2)
    assert all(v.shape == (512, 512, 3) for v in gpu.values())
    csv = (d / "host.csv").read_text()
    assert "psnr_y" in csv and len(csv.splitlines()) >= 3 and (d / "gpu.csv").read_text() == csv


def test_eval_batch_center_crop_gpu_writes_the_host_files(tmp_path):
    """eval_batch.py --degrade --save_lq at --image_size 512 (the smallest --degrade takes): --center_crop gpu --jpeg_decoder gpu writes the
    results, condition images and LQ crops of --center_crop host."""
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _decode_tree
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "photos" / "sub", exist_ok=True)
    Image.fromarray(_photo_like(600, 700, 5)).save(d / "photos" / "a.jpg", quality=92)
    Image.fromarray(_photo_like(1300, 1100, 6)).save(d / "photos" / "sub" / "b.png")
    Image.fromarray(_photo_like(520, 512, 7)).save(d / "photos" / "c.jpg", quality=85, subsampling="4:4:4")
    trees = {}
    for name, extra in (("host", ["--center_crop", "host"]), ("gpu", ["--center_crop", "gpu", "--jpeg_decoder", "gpu"])):
        out = _run([sys.executable, os.path.join(ROOT, "eval_batch.py"), "--input", str(d / "photos"), *_models(d), "--output", str(d / name / "res"),
                    "--cond_output", str(d / name / "cond"), "--batch_size", "2", "--image_size", "512", "--workers", "2", "--degrade", "--degrade_seed", "5",
                    "--save_lq", str(d / name / "lq"), *extra])
        trees[name] = _decode_tree(d / name)
        if name == "gpu":
            assert "2 of 3 files were decoded on the device" in out, out[-1500:]
    _same_trees(trees["host"], trees["gpu"], 9)
    assert all(v.shape == (512, 512, 3) for v in trees["gpu"].values())
