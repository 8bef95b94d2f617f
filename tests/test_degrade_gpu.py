"""ir_degrade (csrc/degrade.hip) through the C ABI and the pipeline against the numpy model, tools/degrade_folder.py.

The gate is equality of bytes - the LQ image and the bytes behind the JPEG step - with no tolerance: every step of the chain is either integer
arithmetic or a fixed sequence of IEEE operations that the model performs in the same order. The JPEG stage is also held to Pillow (libjpeg)
itself, so the kernel is pinned to the library and not only to the model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from instarevive_amd import _lib as L
from instarevive_amd import degrade as D
from tests.support import degrade_model as DM
from tools import degrade_folder as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xA5


def _ctx():
    from instarevive_amd.models import get_context
    return get_context(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def device_results():
    """{case: (LQ images, bytes behind the JPEG step)} - every variant of a case in ONE call, a batch of twelve records; computed once."""
    out = {}
    for name, h, w, _, _ in DM.CASES:
        ps = DM.params(name)
        out[name] = D.degrade(_ctx(), [DM.image(h, w)] * len(ps), ps, with_jpeg=True)
    return out


@pytest.mark.parametrize("name", [c[0] for c in DM.CASES])
def test_bytes_equal_the_model(name, device_results):
    lq, mid = device_results[name]
    for i, ((q, nz, norm), (m_lq, m_mid, _)) in enumerate(zip(DM.VARIANTS, DM.model(name))):
        what = f"{name} q {q} noise {nz} norm {norm}"
        d_mid = int(np.abs(mid[i].astype(int) - m_mid).max())
        d_lq = int(np.abs(lq[i].astype(int) - m_lq).max())
        print(f"{what}: largest byte difference behind JPEG {d_mid}, of the LQ image {d_lq}")
        assert np.array_equal(mid[i], m_mid), (what, np.argwhere(mid[i] != m_mid)[:4])
        assert np.array_equal(lq[i], m_lq), (what, np.argwhere(lq[i] != m_lq)[:4])
    norms = {v: i for i, v in enumerate(DM.VARIANTS)}
    assert not np.array_equal(lq[norms[(60, False, M.NORM_NONE)]], lq[norms[(60, False, M.NORM_MAX)]])   # the blurred image has no white: max brightens it


@pytest.mark.parametrize("name,variant", [("53x37_s2.3", (60, True, M.NORM_NONE)), ("64x41_s4.0", (10, False, M.NORM_NONE)),
                                          ("256x192_s3.1", (100, True, M.NORM_NONE))])
def test_jpeg_stage_equals_pillow(name, variant, device_results):
    """Pillow's own round trip of the bytes ahead of the JPEG step equals what the device left behind it."""
    i = DM.VARIANTS.index(variant)
    ahead = DM.model(name)[i][2]
    assert np.array_equal(device_results[name][1][i], DM.pillow_roundtrip(ahead, variant[0]))


@pytest.mark.parametrize("hw,q", [((23, 16), 60), ((10, 16), 10), ((64, 88), 100), ((61, 83), 35)])
def test_jpeg_stage_alone_equals_pillow(hw, q):
    """A delta kernel at scale 1 without noise hands the image's own bytes to the JPEG step: its output is libjpeg's, no model in between."""
    h, w = hw
    img = np.random.default_rng([h, w, q]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: h // 2] = DM.image(h, w)[: h // 2]
    lq, mid = D.degrade(_ctx(), [img], [D.Params(D.delta_kernel(1), h, w, 0.0, q, None, M.NORM_NONE)], with_jpeg=True)
    ref = DM.pillow_roundtrip(img, q)
    assert np.array_equal(mid[0], ref), np.argwhere(mid[0] != ref)[:4]
    assert np.array_equal(lq[0], ref)   # scale 1 both ways: the resizes are the identity


def test_identity_settings_reproduce_the_input():
    img = DM.image(37, 53)
    for K in (1, 41):
        assert np.array_equal(D.degrade(_ctx(), [img], [D.Params(D.delta_kernel(K), 37, 53, 0.0, 0, None, M.NORM_NONE)])[0], img)


def test_a_batch_equals_its_images_run_singly(device_results):
    """Three different images with different parameters in one call: the bytes of three calls of one image, and of a second batched call."""
    h, w = 48, 40
    imgs = [DM.image(h, w, seed) for seed in (0, 1, 2)]
    ps = [DM.params("48x40_s2.0")[DM.VARIANTS.index(v)] for v in ((10, True, M.NORM_MAX), (100, False, M.NORM_NONE), (60, True, M.NORM_NONE))]
    ps[1] = ps[1]._replace(lh=17, lw=13, kernel=DM.kernel((7, 1.3, 1.3, 0.0, True)))
    ps[2] = ps[2]._replace(q=0)
    lq, mid = D.degrade(_ctx(), imgs, ps, with_jpeg=True)
    for i in range(3):
        one_lq, one_mid = D.degrade(_ctx(), [imgs[i]], [ps[i]], with_jpeg=True)
        assert np.array_equal(lq[i], one_lq[0]), i
        assert (mid[i] is None and one_mid[0] is None) or np.array_equal(mid[i], one_mid[0]), i
        assert np.array_equal(lq[i], M.degrade_model(imgs[i], ps[i].kernel, ps[i].lh, ps[i].lw, ps[i].sigma, ps[i].q, ps[i].noise, ps[i].norm)), i
    again, _ = D.degrade(_ctx(), imgs, ps, with_jpeg=True)
    assert all(np.array_equal(a, b) for a, b in zip(lq, again))
    assert np.array_equal(lq[0], device_results["48x40_s2.0"][0][DM.VARIANTS.index((10, True, M.NORM_MAX))])


def test_embedded_images_with_rows_and_pitch_and_exact_workspace():
    """rows > h and pitch > 3 w: the same bytes, nothing outside the h x w rectangles or behind the stated workspace is written."""
    ctx = _ctx()
    name, h, w = "37x53_s2.3", 37, 53
    rows, pitch = h + 5, 3 * w + 29
    i = DM.VARIANTS.index((60, True, M.NORM_MAX))
    p = DM.params(name)[i]
    buf = np.random.default_rng(3).integers(0, 256, (2, rows, pitch), dtype=np.uint8)
    for k in range(2):
        buf[k, :h, :3 * w] = DM.image(h, w).reshape(h, -1)
    src = torch.from_numpy(buf).cuda()
    out = torch.full((2, rows, pitch), CANARY, dtype=torch.uint8, device="cuda")
    kern, noise = torch.from_numpy(p.kernel).cuda(), torch.from_numpy(p.noise).cuda()
    need = ctx.ws_bytes(L.STAGE_DEGRADE, 2, h, w)
    assert need == D.ws_bytes(h, w) > 0
    raw = torch.full((need + 256 + 64,), CANARY, dtype=torch.uint8, device="cuda")
    off = -raw.data_ptr() % 256
    recs = (L.DegradeParams * 2)(D.record(p, kern.data_ptr(), noise.data_ptr()), D.record(p, kern.data_ptr(), noise.data_ptr()))
    ctx.check(ctx.lib.ir_degrade(ctx.h, ctx.stream(), L.ptr(src), rows, pitch, 2, h, w, recs, L.ptr(out), None,
                                 C.c_void_p(raw.data_ptr() + off), need), "ir_degrade")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = DM.model(name)[i][0]
    for k in range(2):
        assert np.array_equal(got[k, :h, :3 * w].reshape(h, w, 3), want)
        assert np.all(got[k, h:] == CANARY) and np.all(got[k, :, 3 * w:] == CANARY)
    r = raw.cpu().numpy()
    assert np.all(r[:off] == CANARY) and np.all(r[off + need:] == CANARY), "bytes outside the stated workspace were written"


def test_bad_arguments_are_refused_and_write_nothing():
    ctx = _ctx()
    h, w = 48, 40
    p = DM.params("48x40_s2.0")[0]
    src = torch.from_numpy(DM.image(h, w)).cuda()
    out = torch.full((h * w * 3,), CANARY, dtype=torch.uint8, device="cuda")
    kern, noise = torch.from_numpy(p.kernel).cuda(), torch.from_numpy(DM.noise(p.lh, p.lw)).cuda()
    need = D.ws_bytes(h, w)
    raw = torch.full((need + 512,), CANARY, dtype=torch.uint8, device="cuda")
    ws = raw.data_ptr() + (-raw.data_ptr() % 256)

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(src), po=L.ptr(out), pw=ws, wsb=need, rec=True, **change):
        r = D.record(p, kern.data_ptr(), noise.data_ptr())
        for k, v in change.items():
            setattr(r, k, v)
        arr = (L.DegradeParams * 1)(r) if rec else None
        return ctx.lib.ir_degrade(ctx.h, ctx.stream(), pi, rows, pitch, n, hh, ww, arr, po, None,
                                  C.c_void_p(pw) if pw else None, wsb)

    refused = {
        "null image": call(pi=None), "null output": call(po=None), "null workspace": call(pw=0), "null records": call(rec=False),
        "null kernel": call(kernel=None), "no images": call(n=0), "h above rows": call(rows=h - 1), "short pitch": call(pitch=3 * w - 1),
        "too small for the blur": call(hh=20, rows=20, lh=8), "too narrow for the blur": call(ww=20, pitch=60, lw=8),
        "even kernel": call(ksize=40), "kernel above 41": call(ksize=43),
        "lh below 8": call(lh=7), "lw below 8": call(lw=7), "lh above h": call(lh=h + 1), "lw above w": call(lw=w + 1),
        "q below 0": call(q=-1), "q above 100": call(q=101), "unknown norm": call(norm=2),
        "short workspace": call(wsb=need - 1), "misaligned workspace": call(pw=ws + 128, wsb=need),
    }
    torch.cuda.synchronize()
    assert all(rc == -1 for rc in refused.values()), {k: v for k, v in refused.items() if v != -1}
    assert bool((out == CANARY).all()), "a refused call wrote to the output"
    assert b"ir_degrade" in ctx.lib.ir_last_error(ctx.h)
    assert call() == 0   # and the arguments they were varied from are accepted
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(h, w, 3), DM.model("48x40_s2.0")[0][0])


# ---------------------------------------------------------------------------------------------------------------- pipeline
def test_process_degrade_equals_a_run_on_the_models_lq_image():
    """process(resize=, degrade=) at the smallest network size, one 64 x 64 ground truth: the LQ image handed to lq_sink is the model's, and
    the results and scores are those of a run that is fed that LQ image as a plain input."""
    from instarevive_amd.pipeline import process
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    gt = DM.image(64, 64, 4)
    p = D.draw(D.load_recipe("lq"), "a/b.png", 64, 64, 231)
    geo = job_geometry((64, 64), 1, True, 64)
    assert geo.net_hw == (64, 64)
    box = []
    preds, st1, scores = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(gt, geo)], degrade=[p], lq_sink=box.append, gt=[gt], **kw)
    want = M.degrade_model(gt, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)
    assert len(box) == 1 and len(box[0]) == 1 and np.array_equal(box[0][0], want)
    assert not np.array_equal(want, gt)
    plain, plain1, plain_scores = process(dit, None, 1, "wavelet", False, False, 64, 32, resize=[ResizeJob(want, geo)], gt=[gt], **kw)
    assert np.array_equal(preds[0], plain[0]) and np.array_equal(st1[0], plain1[0])
    assert scores == plain_scores
    with pytest.raises(ValueError, match="needs resize"):
        process(dit, [gt], 1, "wavelet", False, False, 64, 32, degrade=[p], **kw)


def test_process_stream_degrade_in_batches():
    """Two batches (two files of different sizes, then one that is enlarged) through process_stream: every LQ image is the model's, in the batches' order."""
    from instarevive_amd.pipeline import process_stream
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.test_models_gpu import DIT_SMALL, _prompt, _small_models
    (sw, _), (vae, _), (dit, _) = _small_models()
    y, mask3 = _prompt(DIT_SMALL)
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    rec = D.load_recipe({"norm": "max"})
    sizes = [[(50, 64), (64, 100)], [(64, 40)]]   # the first two reach one network input, 64 x 128, from different sizes
    gts = [[DM.image(h, w, 9) for h, w in row] for row in sizes]
    ps = [[D.draw(rec, f"{b}_{i}.png", h, w, 5) for i, (h, w) in enumerate(row)] for b, row in enumerate(sizes)]
    records = [[ResizeJob(g, job_geometry((g.shape[1], g.shape[0]), 1, True, 64)) for g in row] for row in gts]
    assert [r.geo.net_hw for r in records[0]] == [(64, 128), (64, 128)]
    box = []
    out = list(process_stream(dit, gts, "wavelet", False, False, 64, 32, return_stage1=False, resize=records, degrade=ps, lq_sink=box.append, **kw))
    assert len(out) == 2 and [len(b) for b in box] == [2, 1]
    for lqs, row, prow in zip(box, gts, ps):
        for lq, g, p in zip(lqs, row, prow):
            assert np.array_equal(lq, M.degrade_model(g, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm))
    plain = list(process_stream(dit, gts, "wavelet", False, False, 64, 32, return_stage1=False, resize=[[ResizeJob(lq, r.geo) for lq, r in zip(lqs, row)]
                                                                                                       for lqs, row in zip(box, records)], **kw))
    for (a, _), (b, _) in zip(out, plain):
        assert all(np.array_equal(x, z) for x, z in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_degrade_saves_the_models_lq_and_scores_like_a_run_on_it(tmp_path):
    """inference.py --degrade --save_lq on a ground-truth folder, then a plain run on the saved LQ folder with --gt: the LQ files hold the
    model's pixels for the parameters the file names draw, and both runs write the same results and the same metrics."""
    import subprocess
    import sys
    from PIL import Image
    from tests.test_cli_gpu import _write_artifacts
    from tests.test_png_gpu import _decode_tree
    d = tmp_path
    _write_artifacts(d)
    for f in (d / "in").glob("**/*"):
        if f.is_file():
            f.unlink()
    files = {"a.png": DM.image(64, 80, 1), "sub/b.png": DM.image(96, 64, 2)}
    for name, img in files.items():
        (d / "in" / name).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(img).save(d / "in" / name)

    def run(out, src, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / src), "--output",
               str(d / out), "--swinir_ckpt", str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"),
               "--dit_config", str(d / "pixart"), "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout

    run("out_deg", "in", "--degrade", "--degrade_seed", "77", "--save_lq", str(d / "lq"), "--metrics_out", str(d / "deg.csv"))
    rec = D.load_recipe("lq")
    for name, img in files.items():
        p = D.draw(rec, name, img.shape[0], img.shape[1], 77)
        saved = np.asarray(Image.open(d / "lq" / name).convert("RGB"))
        assert np.array_equal(saved, M.degrade_model(img, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)), name
    run("out_plain", "lq", "--resize", "gpu", "--gt", str(d / "in"), "--metrics_out", str(d / "plain.csv"))
    a, b = _decode_tree(d / "out_deg"), _decode_tree(d / "out_plain")
    assert sorted(a) == sorted(b) and len(a) == 2 and all(np.array_equal(a[k], b[k]) for k in a)
    assert (d / "deg.csv").read_text() == (d / "plain.csv").read_text() and "psnr_y" in (d / "deg.csv").read_text()
    for flag in ("--show_lq", "--use_center_crop"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", "x", "--input", str(d / "in"), "--output", str(d / "no"), "--degrade", flag],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode != 0 and f"cannot be combined with {flag}" in r.stderr, r.stderr[-500:]
