#!/usr/bin/env python3
"""MUSIQ on the device (ir_musiq, --musiq_model) measured against the host model of the same tree (tools/evaluate_musiq.py), with seeded weights
at the real shapes (hidden 384, MLP 1152, 6 heads, 14 layers; the pretrained file does not exist offline):

  1. The algorithmic cost, counted from the definition: multiply-accumulates of the patch stem, the embedding and the transformer, and the time
     they take at the fp32-MFMA peak.
  2. HIP-event time of ir_musiq for one 2048 x 2048 result and for a batch of four 512 x 512 results, with warm-up, `--repeats` timed event
     pairs of BATCH calls over rotating inputs, the fraction of the fp32 floor reached, next to the network step (events around ir_pipeline
     alone) measured in the same process. Every result is compared with the fp32 CPU model before it is timed.
  3. The CPU fp32 model's time for the same images.
  4. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs):
     three runs without --musiq_model, on --baseline_root (a built checkout of the parent commit; default this tree), then three runs with it
     on this tree. The allowance of the comparison is the baseline's own run-to-run spread (max - min of its three runs); both are printed.

    python tools/bench_musiq.py [--files 16] [--repeats 10] [--skip_cli] [--skip_host_2048] [--baseline_root DIR] [--out FILE]"""
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
from tools.bench_clipiqa import _image  # noqa: E402
from tools import evaluate_musiq as EM  # noqa: E402

EDGE = 2048
BATCH = 4
SHAPES = [(2048, 1), (512, 4)]   # (edge, n)
PEAK_FP32_MFMA = 157.3e12        # FLOP/s of v_mfma_f32_32x32x2_f32 on an MI355X
CFG = dict(patch=EM.PATCH, hidden=384, mlp=1152, heads=6, layers=14, grid=EM.GRID, longer=EM.LONGER)


def seeded_model(seed=8765):
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in EM.model_keys(CFG).items():
        norm = ".gn" in k or ".ln" in k or k.startswith("final_ln")
        if len(shape) == 4 or k in ("position_emb", "scale_emb", "cls_token"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) == 2:
            sd[k] = torch.randn(shape, generator=g) * shape[1] ** -0.5
        elif norm and k.endswith(".weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    return EM.load_model(sd)


def macs(h, w):
    """(patch stem, embedding, transformer) multiply-accumulates of one h x w image."""
    T = EM.layout(h, w)[2]
    P, C, M = T - 1, CFG["hidden"], CFG["mlp"]
    stem = P * (256 * 147 * 64 + 64 * (64 * 64 + 576 * 64 + 2 * 64 * 256))
    emb = P * 8 * 8 * 256 * C
    trans = CFG["layers"] * (T * (4 * C * C + 2 * C * M) + 2 * T * T * C)
    return stem, emb, trans


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L, musiq
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    for edge, n in SHAPES:
        s, e, t = macs(edge, edge)
        say(f"algorithmic cost of one {edge} x {edge} image (T = {EM.layout(edge, edge)[2]}): patch stem {2 * s / 1e9:.1f} GFLOP + embedding {2 * e / 1e9:.1f} + "
            f"transformer {2 * t / 1e9:.1f} = {2 * (s + e + t) / 1e9:.0f} GFLOP; {1e3 * 2 * (s + e + t) / PEAK_FP32_MFMA:.2f} ms at the "
            f"{PEAK_FP32_MFMA / 1e12:.1f} TF fp32-MFMA peak")
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
    model = seeded_model()
    musiq.configure(ctx, model)
    for edge, n in SHAPES:
        img = _image(edge, edge)
        want = None
        if edge < 2048 or not a.skip_host_2048:
            t0 = time.perf_counter()
            want = EM.musiq(img, model)
            t1 = time.perf_counter()
            say(f"CPU fp32 model (tools/evaluate_musiq.py, torch, {torch.get_num_threads()} threads) on one {edge} x {edge} image: {t1 - t0:.3f} s"
                + (f"; a batch of {n}: {n * (t1 - t0):.3f} s" if n > 1 else ""))
        else:
            say(f"CPU fp32 model on one {edge} x {edge} image: not measured (--skip_host_2048)")
        need = musiq.ws_bytes(ctx, n, edge, edge)
        say(f"workspace of ir_musiq for n = {n} of {edge} x {edge}: {need} bytes")
        rotate = 2
        t = torch.from_numpy(img).to(device)
        ins = [t.expand(n, -1, -1, -1).contiguous() for _ in range(rotate)]
        out = torch.zeros((n,), dtype=torch.float64, device=device)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_musiq(ctx.h, ctx.stream(), L.ptr(ins[k]), edge, 3 * edge, n, edge, edge, L.ptr(out), None, L.ptr(ws), ws.numel()), "ir_musiq")
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        got = out.cpu().tolist()
        assert all(v == got[0] for v in got), got
        dev = abs(got[0] - want) if want is not None else float("nan")
        assert want is None or dev < 1e-4, (got[0], want)
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
        floor = 1e3 * n * 2 * sum(macs(edge, edge)) / PEAK_FP32_MFMA
        say(f"ir_musiq {edge} x {edge}, n = {n} ({rotate} rotating inputs, per call of {BATCH} per event pair; score {got[0]:.9f}, "
            f"{'%.1e from the CPU fp32 model' % dev if want is not None else 'not compared'}): {spread(ms)}; {100 * floor / med:.1f} % of the fp32 floor "
            f"({floor:.2f} ms); per image {100 * med / n / step:.1f} % of the {EDGE} x {EDGE} step's {step:.2f} ms")
        del ins, ws
    return sds, model


def cli_leg(a, sds, model):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_musiq_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        EM.save_npz(os.path.join(d, "musiq.npz"), model)
        for how in ("base", "base", "base", "musiq", "musiq", "musiq"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu"] + (["--musiq_model", os.path.join(d, "musiq.npz")] if how == "musiq" else []) + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith("musiq: "))
            say(f"{'with --musiq_model   ' if how == 'musiq' else 'without --musiq_model'} ({'this tree' if root == ROOT else 'the parent commit, built'}): "
                f"{c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("musiq"):
        base, mine = rates["base"], rates["musiq"]
        spread_base = max(base) - min(base)
        say(f"--musiq_model {[round(v, 3) for v in mine]} files/s, without (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is {spread_base:.3f} "
            f"files/s ({100 * spread_base / statistics.median(base):.1f} %); median with the flag {statistics.median(mine):.3f} against "
            f"{statistics.median(base):.3f} ({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--skip_host_2048", action="store_true", help="do not time the CPU model at 2048 x 2048")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --musiq_model (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    try:
        sds, model = kernel_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds, model)
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
