#!/usr/bin/env python3
"""The device part of NIQE (ir_niqe_stats, --niqe_params) measured against the host model of the same tree (tools/evaluate_niqe.py):

  1. HIP-event time of ir_niqe_stats for one 2048 x 2048 result and for a batch of four 512 x 512 results, with warm-up, `--repeats` timed event
     pairs of BATCH calls over rotating inputs that together exceed the last-level cache, next to the network step (events around ir_pipeline
     alone) measured in the same process. Every result is compared with the host model before it is timed (counts equal, sums within 1e-10).
  2. The host model's time for the same images (steps 1-7, numpy fp64, one thread) and the time of the host part that stays on the host
     (niqe.features_from_stats + niqe.score: the fits and the score from the downloaded statistics).
  3. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs):
     three runs without --niqe_params, on --baseline_root (a built checkout of the parent commit; default this tree), then three runs with it
     on this tree. The allowance of the comparison is the baseline's own run-to-run spread (max - min of its three runs); both are printed.

    python tools/bench_niqe.py [--files 16] [--repeats 20] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

EDGE = 2048
BATCH = 8
LAST_LEVEL_CACHE = 256 << 20
SHAPES = [(2048, 1), (512, 4)]   # (edge, n)


def _model():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_niqe", os.path.join(ROOT, "tools", "evaluate_niqe.py"))
    en = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(en)
    return en


def _image(edge, seed):
    """A smooth image with sigma-3 noise and one saturated patch (a photograph's sky)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    img = np.clip(np.rint(base + rng.normal(0, 3.0, base.shape)), 0, 255).astype(np.uint8)
    img[edge // 16:edge // 4, edge // 8:edge // 2] = 255
    return img


def _pristine(en):
    """Seeded stand-in parameters (no niqe_modelparameters.mat exists offline): the features of a seeded image."""
    feat = en.block_features(en.image_stats(_image(480, 7)))
    return feat.mean(axis=0), np.cov(feat, rowvar=False, ddof=1) + 1e-3 * np.eye(36)


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L, niqe
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    device = torch.device("cuda", 0)
    swin, vae, dit, sched, sds = bench.build_models(device, say)
    y, mask = bench.synthetic_prompt()
    lq = bench.upscale_bicubic(bench.synthetic_lq(1, 512, 512, 500), 4)
    ctx = dit.ctx
    st = _Staging.get(ctx, 1, EDGE, EDGE)
    st.fill(0, [lq[0].numpy()])
    st.upload(0)
    _prepare_fused(dit, y.to(device), mask.to(device), EDGE, EDGE, False, 512, (vae, swin))
    flags = _pipeline_flags(dit, "wavelet", False, False)
    acp, sf = float(sched.alphas_cumprod[400]), float(vae.config.scaling_factor)
    step_ms = []
    for i in range(a.step_repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _launch_pipeline(ctx, st, 0, 1, EDGE, EDGE, flags, 512, 448, acp, sf, False)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            step_ms.append(e0.elapsed_time(e1))
    say(f"network step at {EDGE} x {EDGE} (ir_pipeline alone, input resident on the device): {spread(step_ms)}")
    del st
    step = statistics.median(step_ms)
    en = _model()
    params = _pristine(en)
    for edge, n in SHAPES:
        img = _image(edge, edge)
        t0 = time.perf_counter()
        want = en.image_stats(img)
        t1 = time.perf_counter()
        want_score = en.score_features(en.block_features(want), *params)
        t2 = time.perf_counter()
        say(f"host model (tools/evaluate_niqe.py, numpy fp64, one thread) on one {edge} x {edge} image: steps 1-5 {t1 - t0:.3f} s, steps 6-7 {t2 - t1:.3f} s"
            + (f"; a batch of {n}: {n * (t2 - t0):.3f} s" if n > 1 else ""))
        nb = niqe.blocks_of(edge, edge)
        moved = 3 * edge * edge * n
        rotate = max(2, -(-LAST_LEVEL_CACHE // moved) + 1)   # the inputs in rotation exceed the last-level cache
        t = torch.from_numpy(img).to(device)
        ins = [t.expand(n, -1, -1, -1).contiguous() for _ in range(rotate)]
        out = torch.zeros((n * nb * niqe.STATS,), dtype=torch.float64, device=device)
        ws = torch.empty(niqe.ws_bytes(n, edge, edge), dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_niqe_stats(ctx.h, ctx.stream(), L.ptr(ins[k]), edge, 3 * edge, n, edge, edge, L.ptr(out), L.ptr(ws), ws.numel()), "ir_niqe_stats")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n, 2, nb, 5, 6)
        dev = 0.0
        for g in got:
            assert np.array_equal(g[..., :2], want[..., :2]), "counts differ from the host model"
            dev = max(dev, float(np.max(np.abs(g[..., 2:] - want[..., 2:]) / np.where(want[..., 2:] != 0, np.abs(want[..., 2:]), 1.0))))
        assert dev <= 1e-10, dev
        t0 = time.perf_counter()
        mine = niqe.score(niqe.features_from_stats(got[0]), params)
        host_part = time.perf_counter() - t0
        assert abs(mine - want_score) <= 1e-9 * want_score, (mine, want_score)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / BATCH)
        med = statistics.median(ms)
        say(f"ir_niqe_stats {edge} x {edge}, n = {n} ({rotate} rotating inputs, per call of {BATCH} per event pair; counts equal to the host model, sums within "
            f"{dev:.1e}, score {mine:.6f} within 1e-9): {spread(ms)}; per image {100 * med / n / step:.3f} % of the {EDGE} x {EDGE} step's {step:.2f} ms; "
            f"the host part (fits + score of one image, {nb} blocks) {1e3 * host_part:.2f} ms")
        del ins
    return sds, params


def cli_leg(a, sds, params):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_niqe_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        np.savez(os.path.join(d, "pristine.npz"), mu_prisparam=params[0], cov_prisparam=params[1])
        for how in ("base", "base", "base", "niqe", "niqe", "niqe"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu"] + (["--niqe_params", os.path.join(d, "pristine.npz")] if how == "niqe" else []) + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith("niqe: "))
            say(f"{'with --niqe_params   ' if how == 'niqe' else 'without --niqe_params'} ({'this tree' if root == ROOT else 'the parent commit, built'}): "
                f"{c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("niqe"):
        base, mine = rates["base"], rates["niqe"]
        spread_base = max(base) - min(base)
        say(f"--niqe_params {[round(v, 3) for v in mine]} files/s, without (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is {spread_base:.3f} files/s "
            f"({100 * spread_base / statistics.median(base):.1f} %); median with the flag {statistics.median(mine):.3f} against {statistics.median(base):.3f} "
            f"({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %): "
            + ("inside the allowance" if statistics.median(mine) >= statistics.median(base) - spread_base else "OUTSIDE the allowance"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --niqe_params (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    try:
        sds, params = kernel_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds, params)
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
