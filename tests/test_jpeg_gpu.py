"""The device JPEG encoder (csrc/jpeg_encode.hip) through the C ABI, the pipeline and the command line. A baseline JPEG with the standard
Huffman tables and a restart interval is a deterministic function of the pixels, so every check is byte equality: the segment against
tools/jpeg_encode_model.py, the wrapped file against PIL's. The sizes are those of tests/test_jpeg_cpu.py, where the model itself is held
against PIL and the set's coverage (ZRL, 63rd coefficient, stuffing, dummy blocks, restart markers) is asserted."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from instarevive_amd.jpeg import RESTART_MCUS, wrap_jpeg
from tests.test_jpeg_cpu import SIZES, content, pil_file, restarts_of
from tools.jpeg_encode_model import encode_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5
QUALITIES = (1, 75, 100)


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


def _encode(buf: np.ndarray, vh: int, vw: int, q: int, sub: int, restart: int, pitch_pad: int = 0, slack: int = 64):
    """ir_jpeg_encode on buf [n][h][w][3] (rows padded by pitch_pad bytes of 0xEE) -> (segments, the whole output buffer, stride, info). The
    output buffer is filled with a canary first."""
    ctx = _ctx()
    n, h, w, _ = buf.shape
    rows = np.full((n, h, 3 * w + pitch_pad), 0xEE, np.uint8)
    rows[:, :, :3 * w] = buf.reshape(n, h, 3 * w)
    d_img = torch.from_numpy(rows).cuda()
    bound = int(ctx.lib.ir_jpeg_bound(vh, vw, sub, restart))
    assert bound > 0
    stride = bound + slack
    d_out = torch.full((n * stride + slack,), CANARY, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_JPEG, n, vh, vw, sub, restart), dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_jpeg_encode(ctx.h, ctx.stream(), L.ptr(d_img), n, h, w, 3 * w + pitch_pad, vh, vw, q, sub, restart, L.ptr(d_out), stride,
                                     L.ptr(d_info), L.ptr(ws), ws.numel()), "ir_jpeg_encode")
    torch.cuda.synchronize()
    out, sizes = d_out.cpu().numpy(), d_info.cpu().numpy().tolist()
    assert all(0 < s <= bound for s in sizes), (sizes, bound)
    return [out[i * stride:i * stride + sizes[i]].tobytes() for i in range(n)], out, stride, sizes


def _assert_canary(out, stride, sizes):
    for i, size in enumerate(sizes):
        assert np.all(out[i * stride + size:(i + 1) * stride] == CANARY), f"image {i}: bytes behind the segment's end were written"
    assert np.all(out[len(sizes) * stride:] == CANARY)


@pytest.mark.parametrize("h,w", SIZES)
def test_segment_equals_the_model_and_the_file_equals_pils(h, w):
    """Both contents, both subsamplings, qualities 1 / 75 / 100 and the four restart intervals of the CPU test, all images of a size in one
    batch per parameter set."""
    imgs = content(h, w)
    buf = np.stack(imgs)
    for sub in (0, 2):
        for q in QUALITIES:
            for restart, pil_kw in restarts_of(w, sub):
                segs, out, stride, sizes = _encode(buf, h, w, q, sub, restart)
                _assert_canary(out, stride, sizes)
                for img, seg in zip(imgs, segs):
                    want = encode_model(img, q, sub, restart)
                    assert seg == want, f"{h} x {w} q {q} subsampling {sub} restart {restart}: {len(seg)} bytes, the model has {len(want)}"
                    assert wrap_jpeg(seg, w, h, q, sub, restart) == pil_file(img, q, sub, **pil_kw)


def test_batch_of_three_valid_rectangles_in_padded_buffers():
    """33 x 70 of 40 x 80 buffers with a pitch of 3 w + 7: the padding differs between the images and must not reach the files; info is right
    per image and nothing behind a segment's end is written, up to the next slot."""
    rng = np.random.default_rng(21)
    vh, vw = 33, 70
    valid = [content(vh, vw)[0], content(vh, vw)[1], rng.integers(0, 256, (vh, vw, 3), dtype=np.uint8)]
    buf = np.stack([rng.integers(0, 256, (40, 80, 3), dtype=np.uint8) for _ in range(3)])
    assert not np.array_equal(buf[0, vh:], buf[1, vh:])
    buf[:, :vh, :vw] = np.stack(valid)
    for sub in (0, 2):
        segs, out, stride, sizes = _encode(buf, vh, vw, 75, sub, 5, pitch_pad=7)
        _assert_canary(out, stride, sizes)
        for img, seg, size in zip(valid, segs, sizes):
            assert size == len(seg) and wrap_jpeg(seg, vw, vh, 75, sub, 5) == pil_file(img, 75, sub, restart_marker_blocks=5)
        assert len(set(segs)) == 3


def test_two_calls_give_identical_bytes():
    buf = content(96, 272)[0][None]
    a = _encode(buf, 96, 272, 95, 2, RESTART_MCUS)[0]
    b = _encode(buf, 96, 272, 95, 2, RESTART_MCUS)[0]
    assert a == b


def test_noise_at_quality_100_stays_within_the_bound():
    buf = content(96, 272)[0][None]
    segs, out, stride, sizes = _encode(buf, 96, 272, 100, 0, RESTART_MCUS)
    print(f"noise 96 x 272 at quality 100, 4:4:4: {sizes[0]} bytes = {sizes[0] / (96 * 272):.2f} per pixel, bound {stride - 64}")
    assert sizes[0] <= stride - 64 and segs[0] == encode_model(buf[0], 100, 0, RESTART_MCUS)


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    stride = int(ctx.lib.ir_jpeg_bound(8, 8, 2, 4))
    out = torch.full((stride,), CANARY, dtype=torch.uint8, device="cuda")
    info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ctx.ws_bytes(L.STAGE_JPEG, 1, 8, 8, 2, 4) + 16, dtype=torch.uint8, device="cuda")
    good = dict(img=L.ptr(img), vh=8, vw=8, q=75, sub=2, restart=4, out=L.ptr(out), stride=stride, info=L.ptr(info), ws=L.ptr(ws), wsb=ws.numel() - 16, pitch=24)

    def call(**kw):
        a = dict(good, **kw)
        return ctx.lib.ir_jpeg_encode(ctx.h, ctx.stream(), a["img"], 1, 8, 8, a["pitch"], a["vh"], a["vw"], a["q"], a["sub"], a["restart"], a["out"], a["stride"],
                                      a["info"], a["ws"], a["wsb"])

    bad = [dict(img=None), dict(out=None), dict(info=None), dict(ws=None), dict(vh=9), dict(vh=0), dict(vw=9), dict(vw=0), dict(q=0), dict(q=101),
           dict(sub=1), dict(sub=3), dict(restart=0), dict(restart=65536), dict(stride=stride - 1), dict(wsb=ws.numel() - 17),
           dict(ws=C.c_void_p(ws.data_ptr() + 4)), dict(pitch=23)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(info[0]) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert int(info[0]) > 0


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _process_small():
    """The reduced models of tests/golden/process_small.npz and its two input images."""
    from instarevive_amd.models import AutoencoderKL, SwinIR, Transformer2DModel
    from tests.test_oracle_golden import PROCESS_CASES, _process_small_models
    fx = np.load(os.path.join(ROOT, "tests", "golden", "process_small.npz"))
    sws, svae, _, dsd = _process_small_models()
    swin = SwinIR(img_size=64, patch_size=1, in_chans=3, embed_dim=60, depths=[2, 2], num_heads=[6, 6], window_size=8, mlp_ratio=2, sf=8, img_range=1.0,
                  upsampler="nearest+conv", resi_connection="1conv", unshuffle=True, unshuffle_scale=8)
    swin.load_state_dict(sws, strict=False)
    vae = AutoencoderKL(block_out_channels=(32, 64, 128, 128))
    vae.load_state_dict(svae)
    dit = Transformer2DModel(num_attention_heads=4, attention_head_dim=72, num_layers=2, sample_size=16, caption_channels=64, cross_attention_dim=288)
    dit.load_state_dict(dsd)
    for m in (swin, vae, dit):
        m.to("cuda")
    img_key, _ = PROCESS_CASES["untiled"]
    imgs = list(fx[img_key])[: fx["untiled_pred"].shape[0]]
    return dit, imgs, dict(preprocess_model=swin, vae=vae, y=torch.from_numpy(fx["y"]).cuda(), y_mask=None)


def test_process_jpeg_equals_pil_on_the_raw_result():
    """process(jpeg=...): the files are PIL's encoding of what the same call returns without jpeg - predictions and stage-1 images, both
    subsamplings, a rectangle smaller than the output; then the same under resize=, where the rectangles are the final sizes."""
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, job_geometry
    dit, imgs, kw = _process_small()
    h, w = imgs[0].shape[:2]
    rects = [(h, w)] + [(h - 9, w - 20)] * (len(imgs) - 1)
    args = (1, "wavelet", False, False, 512, 448)
    raw, raw1 = process(dit, imgs, *args, **kw)
    for q, sub in ((95, 2), (60, 444)):
        files, files1 = process(dit, imgs, *args, jpeg=rects, jpeg_quality=q, jpeg_subsampling=sub, **kw)
        assert len(files) == len(files1) == len(imgs)
        for arr, blob, (vh, vw) in list(zip(raw, files, rects)) + list(zip(raw1, files1, rects)):
            assert isinstance(blob, bytes)
            assert blob == pil_file(np.ascontiguousarray(arr[:vh, :vw]), q, 0 if sub == 444 else 2, restart_marker_blocks=RESTART_MCUS)
    with pytest.raises(ValueError):
        process(dit, imgs, *args, jpeg=rects, png=rects, **kw)
    # resize=: an enlarged input is resized back on the device; the file is that final image
    small = np.ascontiguousarray(imgs[0][:40, :56])
    recs = [ResizeJob(small, job_geometry((56, 40), 1, True, 64))]
    final, _ = process(dit, None, *args, return_stage1=False, resize=recs, **kw)
    coded, none = process(dit, None, *args, return_stage1=False, resize=recs, jpeg=[final[0].shape[:2]], **kw)
    assert none == [] and coded[0] == pil_file(final[0], 95, 2, restart_marker_blocks=RESTART_MCUS)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_gpu_and_host_encoders_write_the_same_bytes(tmp_path):
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in" / "deep", exist_ok=True)
    for i, (name, hw) in enumerate((("a.png", (512, 512)), ("deep/b.png", (512, 640)), ("c.png", (40, 56)))):   # two plain crops, one that LANCZOS resizes back
        Image.fromarray((det_input(900 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / name)
    outs = {}
    for enc in ("host", "gpu"):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--output",
               str(d / f"out_{enc}"), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--workers", "2", "--save_format", "jpg", "--jpeg_quality", "90",
               "--jpeg_encoder", enc]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[enc] = {os.path.relpath(os.path.join(root, nm), d / f"out_{enc}"): open(os.path.join(root, nm), "rb").read()
                     for root, _, names in os.walk(d / f"out_{enc}") for nm in names}
        if enc == "gpu":
            note = [ln for ln in r.stdout.splitlines() if "--jpeg_encoder gpu" in ln]
            assert len(note) == 1 and " 2 of 3 files were coded on the device, 1 took the host encoder" in note[0], r.stdout[-1500:]
    assert sorted(outs["host"]) == sorted(outs["gpu"]) == ["a_0.jpg", "c_0.jpg", "deep/b_0.jpg"]
    for k in outs["host"]:
        assert outs["host"][k] == outs["gpu"][k], k
        assert Image.open(io.BytesIO(outs["gpu"][k])).format == "JPEG"
