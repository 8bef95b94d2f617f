#!/usr/bin/env python3
"""The device scorer (ir_metrics_y, --gt) measured against the host model of the same tree (tools/evaluate_pairs.py):

  1. HIP-event time of ir_metrics_y at 2048 x 2048 and 512 x 512 for n = 1 and n = 8, with warm-up, `--repeats` timed event pairs of BATCH calls over
     rotating pairs that together exceed the last-level cache, next to the network step (events around ir_pipeline alone) measured in the same
     process and to the call's HBM floor (6 bytes per pixel over 8 TB/s). Every result is compared with the host model before it is timed.
  2. The host model's time (psnr_y + ssim_y, numpy fp64) for one pair of each size.
  3. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs)
     alternating a run without --gt and a run with --gt against K ground-truth files of 2048 x 2048, in one call, two runs each way. --baseline_root
     names another checkout (the parent commit, built) for the runs without --gt; by default they take this tree.

    python tools/bench_metrics.py [--files 16] [--repeats 20] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
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
HBM_BYTES_PER_S = 8e12
SHAPES = [(2048, 1), (2048, 8), (512, 1), (512, 8)]   # (edge, n)


def _model():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_pairs", os.path.join(ROOT, "tools", "evaluate_pairs.py"))
    ep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ep)
    return ep


def _pair(edge, seed):
    """A smooth image with sigma-3 noise and a partner perturbed by up to +-3 per sample (scores of a restoration's order)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    a = np.clip(np.rint(base + rng.normal(0, 3.0, base.shape)), 0, 255).astype(np.uint8)
    return a, np.clip(a.astype(np.int64) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L
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
    ep = _model()
    host = {}
    for edge in (2048, 512):
        pa, pb = _pair(edge, edge)
        fa, fb = np.asarray(pa, np.float32) / 255.0, np.asarray(pb, np.float32) / 255.0
        t0 = time.perf_counter()
        d = ep.to_y(fa, 1.0) - ep.to_y(fb, 1.0)
        host[edge] = (pa, pb, float(np.mean(d * d)), ep.ssim_y(fa, fb))
        ep.psnr_y(fa, fb)
        say(f"host model (tools/evaluate_pairs.py psnr_y + ssim_y, numpy fp64, one thread) on one {edge} x {edge} pair: {time.perf_counter() - t0:.3f} s")
    for edge, n in SHAPES:
        pa, pb, want_mse, want_ssim = host[edge]
        moved = 6 * edge * edge * n
        rotate = max(2, -(-LAST_LEVEL_CACHE // moved) + 1)   # the pairs in rotation exceed the last-level cache
        ta, tb = torch.from_numpy(pa).to(device), torch.from_numpy(pb).to(device)
        ins = [(ta.expand(n, -1, -1, -1).contiguous(), tb.expand(n, -1, -1, -1).contiguous()) for _ in range(rotate)]
        out = torch.zeros((n, 2), dtype=torch.float64, device=device)
        ws = torch.empty(int(ctx.lib.ir_workspace_bytes(None, L.STAGE_METRICS, n, edge, edge, 0, 0, 0)), dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_metrics_y(ctx.h, ctx.stream(), L.ptr(ins[k][0]), edge, 3 * edge, L.ptr(ins[k][1]), edge, 3 * edge, n, edge, edge, L.ptr(out),
                                           L.ptr(ws), ws.numel()), "ir_metrics_y")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(np.abs(got[:, 1] - want_ssim) <= 1e-9) and np.all(np.abs(got[:, 0] - want_mse) <= 1e-9 * max(want_mse, 1e-8)), (got, want_mse, want_ssim)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / BATCH)
        med, floor = statistics.median(ms), 1e3 * moved / HBM_BYTES_PER_S
        say(f"ir_metrics_y {edge} x {edge}, n = {n} ({rotate} rotating pairs, per call of {BATCH} per event pair; equal to the host model within 1e-9): {spread(ms)}; "
            f"HBM floor {floor:.4f} ms ({moved / 1e6:.1f} MB over 8 TB/s): the call reaches {100 * floor / med:.1f} % of it; per image {100 * med / n / step:.3f} % of the "
            f"{EDGE} x {EDGE} step's {step:.2f} ms")
        del ins
    return sds


def cli_leg(a, sds):
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_metrics_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        os.makedirs(os.path.join(d, "gt"))
        for i in range(a.files):   # ground truth of the saved size (512 x 4); photograph-like, so that its decode costs what a real one costs
            Image.fromarray(_pair(EDGE, 100 + i % 4)[0]).save(os.path.join(d, "gt", f"f{i:03d}.png"), compress_level=1)
        for how in ("base", "gt", "base", "gt"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu"] + (["--gt", os.path.join(d, "gt")] if how == "gt" else []) + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ")))
            say(f"{'with --gt   ' if how == 'gt' else 'without --gt'} ({'this tree' if root == ROOT else root}): {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the "
                f"first result, results left the GPU at {c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("gt"):
        low = min(rates["base"])
        say(f"--gt {rates['gt']} files/s, without {rates['base']}; the lower --gt run is {100 * (min(rates['gt']) / low - 1):+.1f} % against the lower run without")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --gt (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    try:
        sds = kernel_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds)
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
