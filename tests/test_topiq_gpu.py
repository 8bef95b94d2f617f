"""ir_topiq (csrc/topiq.hip) through the C ABI, the pipeline and the command line against the float64 model, tools/evaluate_topiq.py.

The gate (tests/support/topiq_model.py): the score within GATE_FACTOR x the fp32 CPU model's largest absolute deviation from the float64
model over the cases; feat and each of the five level means within GATE_FACTOR x their largest relative L2 deviation.
tests/test_topiq_cpu.py shows that every planted bug misses this gate by more than ten times. No test provokes a fault."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from instarevive_amd import _lib as L
from tests.support import topiq_model as TM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, OUT_CANARY = 0xA5, -777.0
NAMES = [c[0] for c in TM.CASES]


def _ctx(kind="small"):
    """The shared context with the seeded model `kind` bound (re-bound only when the other one was)."""
    from instarevive_amd import topiq
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if ctx.__dict__.get("_test_topiq_kind") != kind:
        topiq.configure(ctx, TM.model(kind))
        ctx.__dict__["_test_topiq_kind"] = kind
    return ctx


def _call(buf: np.ndarray, h: int, w: int, kind="small"):
    """ir_topiq on buf [n][rows][pitch] (bytes) with exactly the workspace reported -> (scores [n], feat [n][D], level means [n][5][D]). The
    outputs have canary values behind them and the workspace 16 canary bytes behind its stated size: all must stay untouched."""
    ctx = _ctx(kind)
    n, rows, pitch = buf.shape
    D = TM.CONFIGS[kind]["dim"]
    dev = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    scores = torch.full((n + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    feat = torch.full((n * D + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    means = torch.full((n * 5 * D + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_TOPIQ, n, h, w, 0, 0)
    assert need > 0
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")
    ctx.check(ctx.lib.ir_topiq(ctx.h, ctx.stream(), L.ptr(dev), rows, pitch, n, h, w, L.ptr(scores), L.ptr(feat), L.ptr(means), L.ptr(ws), need), "ir_topiq")
    torch.cuda.synchronize()
    s, f, m = scores.cpu().numpy(), feat.cpu().numpy(), means.cpu().numpy()
    assert np.all(s[n:] == OUT_CANARY), "values behind scores were written"
    assert np.all(f[n * D:] == OUT_CANARY), "values behind feat were written"
    assert np.all(m[n * 5 * D:] == OUT_CANARY), "values behind level_means were written"
    assert bool((ws[need:] == CANARY).all()), "bytes behind the stated workspace were written"
    return s[:n].copy(), f[:n * D].reshape(n, D).copy(), m[:n * 5 * D].reshape(n, 5, D).copy()


def _tight(imgs):
    a = np.stack(imgs)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(np.asarray(a)), _bits(np.asarray(b)))


def _same3(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def device_results():
    """{case: (score, feat, level means)} of every case, one call each; computed once (the cases of one model together, `small` last so that
    the later tests find it bound)."""
    out = {}
    for name, h, w, kind in sorted(TM.CASES, key=lambda c: c[3]):
        s, f, m = _call(_tight([TM.image(name)]), h, w, kind)
        out[name] = (s[0], f[0], m[0])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_score_feat_and_level_means_are_within_the_gate_of_the_float64_model(name, device_results):
    score, feat, means = device_results[name]
    ds, df = TM.deviations(score, feat, means, name)
    gs, gf = TM.gate()
    hs, hf = TM.host_deviation(name)
    print(f"{name}: topiq_nr {score:.12f} (model {TM.reference(name)[0]:.12f}); score deviation {ds:.3e} (gate {gs:.3e}, host fp32 {hs:.3e})")
    for part, d, g, hd in zip(TM.PARTS, df, gf, hf):
        print(f"    {part}: deviation {d:.3e} (gate {g:.3e}, host fp32 {hd:.3e})")
    assert np.isfinite(score) and ds <= gs
    for part, d, g in zip(TM.PARTS, df, gf):
        assert d <= g, part


def test_the_same_case_twice_gives_the_same_bits_and_a_batch_each_image_its_own(device_results):
    name = "131x97"
    img = TM.image(name)
    one = _call(_tight([img]), 131, 97)
    assert _same3([v[0] for v in one], device_results[name])
    other = TM.ramp(131, 97, 5)
    sb, fb, mb = _call(_tight([other, img, other]), 131, 97)
    assert _same(sb[1], one[0][0]) and _same(fb[1], one[1][0]) and _same(mb[1], one[2][0])
    assert _same(sb[0], sb[2]) and _same(fb[0], fb[2]) and _same(mb[0], mb[2]) and sb[0] != sb[1]


def test_embedded_image_with_rows_and_pitch(device_results):
    """rows > h and pitch > 3 w: the same bits as the tight image."""
    name = "33x40"
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1, 41, 3 * 40 + 37), dtype=np.uint8)
    buf[0, :33, :3 * 40] = TM.image(name).reshape(33, -1)
    got = _call(buf, 33, 40)
    assert _same3([v[0] for v in got], device_results[name])


def test_bad_arguments_are_refused_and_write_nothing(device_results):
    ctx = _ctx()
    name, h, w = "64x64", 64, 64
    D = TM.CONFIGS["small"]["dim"]
    img = torch.from_numpy(TM.image(name)).cuda()
    out = torch.full((1 + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    feat = torch.full((D + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    means = torch.full((5 * D + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_TOPIQ, 1, h, w, 0, 0)
    ws = torch.full((need + 16,), CANARY, dtype=torch.uint8, device="cuda")

    def call(n=1, hh=h, ww=w, rows=h, pitch=3 * w, pi=L.ptr(img), po=L.ptr(out), pf=L.ptr(feat), pm=L.ptr(means), pw=L.ptr(ws), wsb=need, handle=ctx.h):
        return ctx.lib.ir_topiq(handle, ctx.stream(), pi, rows, pitch, n, hh, ww, po, pf, pm, pw, wsb)

    assert call(n=0) == -1
    assert call(hh=15) == -1 and call(ww=15) == -1 and "15" in ctx.lib.ir_last_error(ctx.h).decode()   # a side of 15
    assert call(rows=h - 1) == -1 and call(pitch=3 * w - 1) == -1
    assert ctx.ws_bytes(L.STAGE_TOPIQ, 0, h, w, 0, 0) == 0 and ctx.ws_bytes(L.STAGE_TOPIQ, 1, 15, w, 0, 0) == 0
    assert call(wsb=need - 1) == -1                                       # a short workspace
    assert call(pw=C.c_void_p(ws.data_ptr() + 4)) == -1                   # a misaligned one
    assert call(po=C.c_void_p(out.data_ptr() + 4)) == -1                  # misaligned scores
    assert call(pi=None) == -1 and call(po=None) == -1 and call(pw=None) == -1 and call(handle=None) == -1
    # a context that was never configured: the documented code, and no workspace size
    fresh = L.Context(0)
    assert fresh.ws_bytes(L.STAGE_TOPIQ, 1, h, w, 0, 0) == 0
    assert call(handle=fresh.h) == L.TOPIQ_NOT_CONFIGURED
    assert "not configured" in fresh.lib.ir_last_error(fresh.h).decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_CANARY).all()) and bool((feat == OUT_CANARY).all()) and bool((means == OUT_CANARY).all()) and bool((ws == CANARY).all())
    assert call(pf=None, pm=None) == 0                                    # feat and level_means may be NULL
    torch.cuda.synchronize()
    assert _same(out[:1].cpu().numpy()[0], device_results[name][0])
    assert bool((feat == OUT_CANARY).all()) and bool((means == OUT_CANARY).all())


def test_configure_names_a_missing_or_misshapen_tensor():
    from instarevive_amd import topiq
    fresh = L.Context(0)
    m = TM.model("small")
    depths = (C.c_int * 4)(*m["cfg"]["depths"])

    def conf(width=8, dim=32, heads=2, ffn=64, dp=depths):
        return fresh.lib.ir_topiq_configure(fresh.h, dp, width, dim, heads, ffn)

    assert conf() == -2 and "topiq." in fresh.lib.ir_last_error(fresh.h).decode()
    assert conf(width=6) == -1 and conf(dim=36) == -1 and conf(heads=3) == -1 and "unsupported" in fresh.lib.ir_last_error(fresh.h).decode()
    assert conf(dp=(C.c_int * 4)(2, 0, 1, 1)) == -1
    topiq.configure(fresh, m)
    fresh.upload("topiq.ca.2.norm3.weight", torch.zeros(7))
    assert conf() == -2 and "topiq.ca.2.norm3.weight" in fresh.lib.ir_last_error(fresh.h).decode()
    assert fresh.ws_bytes(L.STAGE_TOPIQ, 1, 64, 64, 0, 0) == 0   # the refused binding left the context unconfigured


def test_rebinding_small_full_small_gives_the_first_bits_again(device_results):
    name = "16x200"
    first = _call(_tight([TM.image(name)]), 16, 200, "small")
    assert _same3([v[0] for v in first], device_results[name])
    full = _call(_tight([TM.image("97x131")]), 97, 131, "full")
    assert _same3([v[0] for v in full], device_results["97x131"])
    again = _call(_tight([TM.image(name)]), 16, 200, "small")
    assert _same3([v[0] for v in again], [v[0] for v in first])


def test_score_arrays_gives_the_calls_bits_and_refuses_a_short_side(device_results):
    from instarevive_amd import topiq
    ctx = _ctx()
    assert topiq.score_arrays(ctx, TM.image("131x97")) == device_results["131x97"][0]
    with pytest.raises(ValueError, match="12 x 200"):
        topiq.score_arrays(ctx, TM.ramp(12, 200, 1))
    assert topiq.scorable(16, 16) and not topiq.scorable(15, 400)


# ---------------------------------------------------------------------------------------------------------------- pipeline
def _model_score(arr):
    """The float64 model's score of an array, NaN where it has none."""
    try:
        return TM.ET.topiq(arr, TM.model("small"), torch.float64)
    except TM.ET.TopiqError:
        return float("nan")


def test_process_scores_the_returned_images():
    """process(topiq=True) on the reduced models: the extra element holds the kernel's score of the image the same call returns - alone, behind
    musiq's value, with gt= (whose rectangle it then scores; a rectangle with a side below 16 gets NaN) and through process_stream."""
    from instarevive_amd import musiq, topiq
    from instarevive_amd.pipeline import process, process_stream
    from tests.golden._det import det_input
    from tests.support import musiq_model as QM
    from tests.support.small_models import small_models
    sw, vae, dit, y = small_models()
    ctx = _ctx()
    assert dit.ctx is ctx
    batch = [(det_input(720 + i, (192, 256, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y)
    gate = TM.gate()[0]
    preds, _, (sp, _) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, topiq=True, **kw)
    assert all(len(t) == 1 for t in sp)
    for (v,), p in zip(sp, preds):
        want = _model_score(p)
        print(f"192 x 256: topiq_nr {v:.12f} (model {want:.12f})")
        assert abs(v - want) <= gate and v == topiq.score_arrays(ctx, p)
    assert len(process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, **kw)) == 2
    musiq.configure(ctx, QM.model())
    p1, _, (sm, _) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, musiq=True, topiq=True, **kw)
    assert all(len(t) == 2 for t in sm)
    for (q, v), p, (v0,) in zip(sm, p1, sp):
        assert v == v0 and q == musiq.score_arrays(ctx, p)
    gts = [TM.ramp(192, 200, 1), TM.ramp(12, 256, 2)]
    p2, _, (sg, _) = process(dit, batch, 1, "wavelet", False, False, 64, 32, return_stage1=False, gt=gts, topiq=True, **kw)
    assert all(len(t) == 3 for t in sg) and abs(sg[0][2] - _model_score(p2[0][:192, :200])) <= gate and np.isnan(sg[1][2])
    out = list(process_stream(dit, [batch, batch[:1]], "wavelet", False, False, 64, 32, return_stage1=False, topiq=True, **kw))
    assert [len(r) for r in out] == [3, 3]
    assert [t for t in out[0][2][0]] == sp and [t for t in out[1][2][0]] == sp[:1]


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli(d, extra, out):
    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
           str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
           "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "2", "--workers", "2", "--output", str(d / out), "--png_encoder", "gpu", "--resize", "gpu"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_cli_topiq_model_writes_the_tools_scores_and_leaves_the_images_alone(tmp_path):
    """inference.py --topiq_model over four small PNGs, one of them 12 pixels high: metrics.csv's topiq_nr column equals
    tools/evaluate_topiq.py --backend gpu over the saved files, the average line is theirs, the short file is counted as not scored; and the
    saved images are byte-equal to a run without the flag."""
    from instarevive_amd.metrics import read_report
    from tests.golden._det import det_input
    from tests.test_cli_gpu import _write_artifacts
    d = tmp_path
    _write_artifacts(d)
    os.makedirs(d / "in")
    for i, hw in enumerate([(72, 80), (96, 80), (128, 66), (12, 64)]):
        Image.fromarray((det_input(860 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / f"im{i}.png")
    TM.ET.save_npz(d / "topiq.npz", TM.model("small"))
    r = _cli(d, ["--topiq_model", str(d / "topiq.npz")], "out")
    text = (d / "out" / "metrics.csv").read_text().splitlines()
    assert text[0] == "file,topiq_nr"
    got = read_report(str(d / "out" / "metrics.csv"))
    assert sorted(got) == ["im0_0.png", "im1_0.png", "im2_0.png"]
    lines = []
    avg, values = TM.ET.evaluate(str(d / "out"), str(d / "topiq.npz"), backend="gpu", log=lines.append)
    for k in got:
        print(f"{k}: topiq_nr {got[k][0]:.12f} (tool {values[k]:.12f})")
        assert values[k] == got[k][0], (k, got[k], values[k])
    assert "im3_0.png" not in values and "(1 not scored)" in lines[-2] and lines[-1] == f"topiq_nr: {avg:.5f}"
    assert f"topiq_nr: {np.mean([v[0] for v in got.values()]):.5f}" in r.stdout.splitlines() and lines[-1] in r.stdout.splitlines()
    assert "--topiq_model: scored 3 files" in r.stdout and "--topiq_model: 1 of 4 files were not scored" in r.stdout, r.stdout[-1500:]
    _cli(d, [], "plain")
    names = sorted(p.name for p in (d / "plain").iterdir())
    assert names == sorted(p.name for p in (d / "out").iterdir() if p.name != "metrics.csv")
    for k in names:
        assert (d / "plain" / k).read_bytes() == (d / "out" / k).read_bytes(), k
