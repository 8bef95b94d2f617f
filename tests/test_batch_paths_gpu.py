"""process() and process_stream() with every optional stage of a batch at once - degrade, the bicubic chain, LANCZOS back, the device PNG encoder,
PSNR-Y / SSIM-Y, LPIPS, NIQE, CLIP-IQA, stage-1 output, lq_sink - and the equivalence of the two entry points, which the feature tests
(test_png_gpu ... test_degrade_gpu) each pin for one stage alone. Nothing is compared with a model here: the gate is equality, element for element,
of what process() returns for a batch and what one process_stream() over the batches yields for it, plain and under graph=True.

lpips= is one switch for a whole process_stream() run, so the plain batch in the middle is scored with LPIPS like its neighbours: every tuple
of the three batches has five values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RUN = ("wavelet", False, False, 64, 32)   # color_fix_type, disable_preprocess_model, tiled, tile_size, tile_stride


def _same_score(a, b):
    return a == b or (a != a and b != b)


def _same_scores(a, b):
    """Two scores elements: pairs of lists of tuples, equal with == and NaN in the same places."""
    return len(a) == len(b) == 2 and all(len(x) == len(y) and all(len(s) == len(t) and all(_same_score(u, v) for u, v in zip(s, t)) for s, t in zip(x, y))
                                         for x, y in zip(a, b))


def _same_images(a, b):
    """Two result lists: PNG files (bytes) or arrays."""
    return len(a) == len(b) and all((x == y) if isinstance(x, bytes) else (not isinstance(y, bytes) and np.array_equal(x, y)) for x, y in zip(a, b))


def _assert_same_batch(got, want, what):
    assert len(got) == len(want) == 3, what
    assert _same_images(got[0], want[0]) and _same_images(got[1], want[1]), what
    assert _same_scores(got[2], want[2]), (what, got[2], want[2])


def test_process_equals_process_stream_with_every_stage_at_once(tmp_path):
    from instarevive_amd import degrade as D
    from instarevive_amd import lpips as LP
    from instarevive_amd.pipeline import process, process_stream
    from instarevive_amd.resample import ResizeJob, job_geometry
    from tests.golden._det import det_input
    from tests.support import clipiqa_model as CM
    from tests.support import degrade_model as DM
    from tests.support import niqe_model as NM
    from tests.support.small_models import small_models
    from tests.test_clipiqa_gpu import _ctx as clipiqa_ctx
    from tests.test_lpips_gpu import _bound, _files
    sw, vae, dit, y = small_models()
    assert clipiqa_ctx() is dit.ctx        # the small CLIP-IQA model is bound to the models' context
    _bound.clear()
    LP.configure(dit.ctx, *_files(tmp_path))   # the synthetic LPIPS weights
    kw = dict(preprocess_model=sw, vae=vae, y=y, lpips=True, niqe=NM.params(), clipiqa=True, return_stage1=True)

    # A and C: an enlarged file (LANCZOS back to 40 x 56) and a plain crop (64 x 90) that reach one network input, 64 x 128; the decoded files
    # are ground truth and are degraded on the device. Every edge is at least 32 (LPIPS and CLIP-IQA score) and below 96 (NIQE gives NaN).
    recipe = D.load_recipe({"norm": "max"})
    sizes = [(40, 56), (64, 90)]

    def resize_batch(seed):
        raws = [DM.image(h, w, seed + i) for i, (h, w) in enumerate(sizes)]
        records = [ResizeJob(g, job_geometry((g.shape[1], g.shape[0]), 1, True, 64)) for g in raws]
        assert [r.geo.lanczos for r in records] == [(56, 40), None] and [r.geo.net_hw for r in records] == [(64, 128), (64, 128)]
        return dict(resize=records, degrade=[D.draw(recipe, f"{seed}_{i}.png", h, w, 5) for i, (h, w) in enumerate(sizes)], png=list(sizes), gt=raws)

    a, c = resize_batch(3), resize_batch(11)
    # B: plain arrays of 192 x 256 with ground truth of the full size; no png, no resize
    b_imgs = [(det_input(820 + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    b_gts = [CM.ramp(192, 256, 1 + i) for i in range(2)]

    box = []
    alone = [process(dit, None, 1, *RUN, lq_sink=box.append, **a, **kw),
             process(dit, b_imgs, 1, *RUN, lq_sink=box.append, gt=b_gts, **kw),
             process(dit, None, 1, *RUN, lq_sink=box.append, **c, **kw)]
    assert [len(lq) for lq in box] == [2, 2]    # once per degraded batch
    for res in (alone[0], alone[2]):
        assert all(isinstance(z, bytes) for z in res[0] + res[1])
        assert all(len(t) == 5 and np.isfinite(t[:3]).all() and np.isnan(t[3]) and np.isfinite(t[4]) for t in res[2][0] + res[2][1]), res[2]
    assert [z.shape for z in alone[1][0] + alone[1][1]] == [(192, 256, 3)] * 4
    assert all(len(t) == 5 and np.isfinite(t).all() for t in alone[1][2][0] + alone[1][2][1]), alone[1][2]
    assert not _same_images(alone[0][0], alone[2][0])

    def stream(**more):
        sink = []
        out = list(process_stream(dit, [[r.raw for r in a["resize"]], b_imgs, [r.raw for r in c["resize"]]], *RUN, lq_sink=sink.append,
                                  png=[a["png"], None, c["png"]], resize=[a["resize"], None, c["resize"]], degrade=[a["degrade"], None, c["degrade"]],
                                  gt=[a["gt"], b_gts, c["gt"]], **more, **kw))
        return out, sink

    for what, more in (("stream", {}), ("stream, graph=True", {"graph": True})):
        out, sink = stream(**more)
        assert len(out) == 3, what
        for k in range(3):
            _assert_same_batch(out[k], alone[k], f"{what}: batch {'ABC'[k]}")
        assert len(sink) == 2 and all(_same_images(s, z) for s, z in zip(sink, box)), what   # A's, then C's
