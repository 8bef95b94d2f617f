#!/usr/bin/env python3
"""The device LPIPS (ir_lpips, --gt with --lpips_lin) measured against the fp32 torch model of the same tree (tools/evaluate_pairs.py::LPIPS), on seeded
random weights at AlexNet's shapes (the pretrained ones do not ship):

  1. `kernel`: HIP-event time of ir_lpips per 2048 x 2048 pair and per batch of four 512 x 512 pairs (eval_batch's shape), with warm-up and
     `--repeats` timed calls over rotating pairs, as a fraction of the fp32-MFMA floor (242.1 / 14.6 GFLOP per pair over 157.3 TF) and next to the
     network step (events around ir_pipeline alone) measured in the same process; the time of every launch of one call (events between them on a
     second pass); the deviation of the 2048 x 2048 result from the host fp32 model, and that model's time for the same pair on 16 CPU threads.
  2. `cli`: files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu --gt as a child process over K synthetic
     512 x 512 PNGs against K ground-truth files of 2048 x 2048) alternating a run without --lpips_lin and a run with it, two runs each way.
     --baseline_root names another checkout (the parent commit, built) for the runs without; by default they take this tree.

Each leg is a child process of its own under `timeout`; a leg that fails ends the run.

    python tools/bench_lpips.py [--files 16] [--repeats 10] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
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
from tools.bench_metrics import _model, _pair  # noqa: E402

EDGE = 2048
PEAK_FLOPS = 157.3e12
STAGE_GFLOP = (12.13, 39.95, 21.40, 28.54, 19.03)   # per 2048 x 2048 image
SHAPES = [(2048, 1), (512, 4)]   # (edge, pairs per call)
LEG_TIMEOUT = {"kernel": 420, "cli": 600}


def random_weights(seed=1234):
    """Seeded random weights at AlexNet's shapes, as (alexnet state dict, lin state dict) in the users' file layout."""
    import torch
    ep = _model()
    g = torch.Generator().manual_seed(seed)
    alex, lin = {}, {}
    for k, (idx, cin, cout, ks, _, _) in enumerate(ep.ALEX_CONVS):
        alex[f"features.{idx}.weight"] = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        alex[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.1
        lin[f"lin{k}.model.1.weight"] = (torch.rand(cout, generator=g) * 2.0 / cout).view(1, cout, 1, 1)
    return alex, lin


def flops_per_pair(edge):
    """Algorithmic FLOPs of the five convolutions for two edge x edge images."""
    ep = _model()
    e, total = edge, 0
    for (_, cin, cout, ks, stride, pad), pool in zip(ep.ALEX_CONVS, ep.ALEX_POOL_BEFORE):
        if pool:
            e = (e - 3) // 2 + 1
        e = (e + 2 * pad - ks) // stride + 1
        total += 2 * e * e * cout * cin * ks * ks
    return 2 * total


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L
    from instarevive_amd import lpips as LP
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    device = torch.device("cuda", 0)
    swin, vae, dit, sched, _ = bench.build_models(device, say)
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
    step = statistics.median(step_ms)
    del st

    alex, lin = random_weights()
    LP.configure(ctx, lin, alex)
    ep = _model()
    net = ep.LPIPS(alex, lin, "cpu")
    torch.set_num_threads(16)
    pa, pb = _pair(EDGE, EDGE)
    fa, fb = (torch.from_numpy(np.asarray(x, np.float32) / 255.0).permute(2, 0, 1)[None] for x in (pa, pb))
    net(fa[:, :, :256, :256], fb[:, :, :256, :256])   # warm the thread pool
    t0 = time.perf_counter()
    want = float(net(fa, fb, normalize=True)[0])
    say(f"host model (tools/evaluate_pairs.py::LPIPS, torch fp32, 16 CPU threads) on one {EDGE} x {EDGE} pair: {time.perf_counter() - t0:.3f} s, lpips {want:.9g}")

    for edge, n in SHAPES:
        rotate = 3
        pairs = [_pair(edge, 10 * edge + k) for k in range(rotate)] if edge != EDGE else [(pa, pb)] + [_pair(edge, 7 + k) for k in range(rotate - 1)]
        ins = [(torch.from_numpy(p[0]).to(device).expand(n, -1, -1, -1).contiguous(), torch.from_numpy(p[1]).to(device).expand(n, -1, -1, -1).contiguous()) for p in pairs]
        out = torch.zeros((n,), dtype=torch.float64, device=device)
        ws = torch.empty(LP.ws_bytes(n, edge, edge), dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            LP.queue_lpips(ctx, ins[k][0].data_ptr(), edge, 3 * edge, ins[k][1].data_ptr(), edge, 3 * edge, n, edge, edge, out, ws)
        call()
        torch.cuda.synchronize()
        if edge == EDGE:
            got = float(out[0])
            say(f"ir_lpips on the same pair: {got:.9g}, off by {abs(got - want) / want:.3e} relative from the host fp32 model")
        for _ in range(2):
            call()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        fl = n * flops_per_pair(edge)
        floor = 1e3 * fl / PEAK_FLOPS
        say(f"ir_lpips {edge} x {edge}, {n} pair(s) per call ({rotate} rotating inputs, workspace {ws.numel() / 1e6:.1f} MB): {spread(ms)}; {fl / 1e9:.1f} GFLOP = "
            f"{fl / med / 1e9:.1f} TF, {100 * floor / med:.1f} % of the {floor:.3f} ms floor at 157.3 TF; per pair {100 * med / n / step:.2f} % of the {EDGE} x {EDGE} "
            f"step's {step:.2f} ms")
        del ins, ws


def cli_leg(a):
    import torch
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_lpips_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        alex, lin = random_weights()
        torch.save(alex, os.path.join(d, "alexnet.pth"))
        torch.save(lin, os.path.join(d, "lin.pth"))
        os.makedirs(os.path.join(d, "gt"))
        for i in range(a.files):
            Image.fromarray(_pair(EDGE, 100 + i % 4)[0]).save(os.path.join(d, "gt", f"f{i:03d}.png"), compress_level=1)
        for how in ("gt", "lpips", "gt", "lpips"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "gt" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu", "--gt", os.path.join(d, "gt")] + flags
            if how == "lpips":
                cmd += ["--lpips_lin", os.path.join(d, "lin.pth"), "--lpips_alexnet", os.path.join(d, "alexnet.pth")]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                raise SystemExit(1)   # nothing more is started on the GPU behind a failed run
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ", "lpips: ")))
            say(f"{'--gt --lpips_lin' if how == 'lpips' else '--gt alone      '} ({'this tree' if root == ROOT else 'the parent commit, built'}): {c['files_per_s']:.2f} files/s overall, "
                f"{c['steady_files_per_s']:.2f} after the first result, results left the GPU at {c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["steady_files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    low = min(rates["gt"])
    say(f"steady files/s: --gt --lpips_lin {rates['lpips']}, --gt alone {rates['gt']}; the lower run with LPIPS is {100 * (min(rates['lpips']) / low - 1):+.1f} % against "
        f"the lower run without")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --lpips_lin (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--leg", default=None, choices=["kernel", "cli"], help=argparse.SUPPRESS)   # the child processes of this tool
    ap.add_argument("--append", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    if a.leg:
        try:
            (kernel_leg if a.leg == "kernel" else cli_leg)(a)
        finally:
            if a.append:
                with open(a.append, "a") as f:
                    f.write("\n".join(LINES) + "\n")
        return 0
    # the driver: one child per leg under its own time limit; a leg that fails, faults or runs out of time ends the run
    fd, log = tempfile.mkstemp(prefix="ir_lpips_bench_", suffix=".txt")
    os.close(fd)
    rc = 0
    try:
        for leg in ["kernel"] + ([] if a.skip_cli else ["cli"]):
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--append", log, "--files", str(a.files),
                   "--repeats", str(a.repeats), "--step_repeats", str(a.step_repeats)] + (["--baseline_root", a.baseline_root] if a.baseline_root else [])
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"leg {leg} ended with status {rc}: stopping", flush=True)
                break
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            shutil.copyfile(log, a.out)
        os.remove(log)
    return rc


if __name__ == "__main__":
    sys.exit(main())
