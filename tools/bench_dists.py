#!/usr/bin/env python3
"""The device DISTS (ir_dists, --gt with --dists_model) measured against the fp32 torch model of the same tree (tools/evaluate_pairs.py::DISTS), on
seeded random weights at VGG-16's widths (the pretrained ones do not ship):

  1. `kernel`: HIP-event time of ir_dists per 2048 x 2048 pair and per batch of four 512 x 512 pairs (eval_batch's shape), with warm-up and
     `--repeats` timed calls over rotating pairs, as a fraction of the fp32-MFMA floor (the algorithmic cost is derived, not measured: 305 856
     MAC per input pixel over the thirteen convolutions, 2.57 TFLOP per 2048 x 2048 image, 5.13 per pair, 32.6 ms at 157.3 TF) and next to
     the network step (events around ir_pipeline alone) measured in the same process; the deviation of a 512 x 512 result from the host fp32
     model, and that model's time for the same pair on 16 CPU threads.
  2. `cli`: files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu --gt as a child process over K synthetic
     512 x 512 PNGs against K ground-truth files of 2048 x 2048), three runs without --dists_model and three with it, alternating. The allowance
     is the spread of the runs without. --baseline_root names another checkout (the parent commit, built) for the runs without; by default
     they take this tree, and the report says which it was.

Each leg is a child process of its own under `timeout`; a leg that fails ends the run.

    python tools/bench_dists.py [--files 8] [--repeats 5] [--skip_cli] [--baseline_root DIR] [--out profiles/dists.txt]"""
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
WIDTHS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)   # how often the map of conv k has been halved
SHAPES = [(2048, 1), (512, 4)]   # (edge, pairs per call)
LEG_TIMEOUT = {"kernel": 420, "cli": 900}


def random_weights(seed=4321):
    """Seeded random weights in ir_dists_configure's names (tests/support/dists_model.py draws the same way)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in range(13):
        cin, cout = WIDTHS[k], WIDTHS[k + 1]
        out[f"dists.c{k + 1}.w"] = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).float()
        out[f"dists.c{k + 1}.b"] = (torch.randn(cout, generator=g) * 0.1).float()
    out["dists.alpha"] = (0.01 + 0.2 * torch.rand(1475, generator=g)).float()
    out["dists.beta"] = (0.01 + 0.2 * torch.rand(1475, generator=g)).float()
    return out


def module_state_dict(w):
    ep = _model()
    sd = {"alpha": w["dists.alpha"].view(1, -1, 1, 1), "beta": w["dists.beta"].view(1, -1, 1, 1)}
    k = 0
    for s, idxs in enumerate(ep.VGG_STAGES):
        for idx in idxs:
            k += 1
            sd[f"stage{s + 1}.{idx}.weight"], sd[f"stage{s + 1}.{idx}.bias"] = w[f"dists.c{k}.w"], w[f"dists.c{k}.b"]
    return sd


def mac_per_pixel():
    """MACs of the thirteen convolutions per input pixel (even sizes): 9 cin cout / 4^level."""
    return sum(9 * WIDTHS[k] * WIDTHS[k + 1] / 4 ** LEVEL[k] for k in range(13))


def flops_per_pair(edge):
    e, total = edge, 0
    for k in range(13):
        if k and LEVEL[k] != LEVEL[k - 1]:
            e = (e + 1) // 2
        total += 2 * e * e * 9 * WIDTHS[k] * WIDTHS[k + 1]
    return 2 * total


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import dists as DD
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    device = torch.device("cuda", 0)
    say(f"derived cost: {mac_per_pixel():.0f} MAC per input pixel, {flops_per_pair(EDGE) / 2e12:.2f} TFLOP per {EDGE} x {EDGE} image, {flops_per_pair(EDGE) / 1e12:.2f} per pair, "
        f"{1e3 * flops_per_pair(EDGE) / PEAK_FLOPS:.1f} ms per pair at the {PEAK_FLOPS / 1e12:.1f} TF fp32 peak")
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

    w = random_weights()
    DD.configure(ctx, w)
    net = _model().DISTS(module_state_dict(w), None, "cpu")
    torch.set_num_threads(16)
    pa, pb = _pair(512, 5120)
    fa, fb = (torch.from_numpy(np.asarray(x, np.float32) / 255.0).permute(2, 0, 1)[None] for x in (pa, pb))
    net(fa[:, :, :64, :64], fb[:, :, :64, :64])   # warm the thread pool
    t0 = time.perf_counter()
    want = float(net(fa, fb)[0])
    cpu_s = time.perf_counter() - t0
    say(f"host model (tools/evaluate_pairs.py::DISTS, torch fp32, 16 CPU threads) on one 512 x 512 pair: {cpu_s:.3f} s (x 16 pixels for a {EDGE} x {EDGE} pair: "
        f"{16 * cpu_s:.1f} s), dists {want:.9g}")

    for edge, n in SHAPES:
        rotate = 2
        pairs = [(pa, pb), _pair(edge, 10 * edge + 1)] if edge == 512 else [_pair(edge, 7 + k) for k in range(rotate)]
        ins = [(torch.from_numpy(p[0]).to(device).expand(n, -1, -1, -1).contiguous(), torch.from_numpy(p[1]).to(device).expand(n, -1, -1, -1).contiguous()) for p in pairs]
        out = torch.zeros((n,), dtype=torch.float64, device=device)
        ws = torch.empty(DD.ws_bytes(n, edge, edge), dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            DD.queue_dists(ctx, ins[k][0].data_ptr(), edge, 3 * edge, ins[k][1].data_ptr(), edge, 3 * edge, n, edge, edge, out, ws)
        call()
        torch.cuda.synchronize()
        if edge == 512:
            got = float(out[0])
            say(f"ir_dists on the same pair: {got:.9g}, off by {abs(got - want):.3e} absolute from the host fp32 model")
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
        say(f"ir_dists {edge} x {edge}, {n} pair(s) per call ({rotate} rotating inputs, workspace {ws.numel() / 1e6:.1f} MB): {spread(ms)}; {fl / 1e9:.1f} GFLOP = "
            f"{fl / med / 1e9:.1f} TF, {100 * floor / med:.1f} % of the {floor:.3f} ms floor at 157.3 TF; per pair {100 * med / n / step:.2f} % of the {EDGE} x {EDGE} "
            f"step's {step:.2f} ms")
        del ins, ws


def cli_leg(a):
    import torch
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_dists_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        np.savez(os.path.join(d, "dists.npz"), **{k: v.numpy() for k, v in random_weights().items()})
        os.makedirs(os.path.join(d, "gt"))
        for i in range(a.files):
            Image.fromarray(_pair(EDGE, 100 + i % 4)[0]).save(os.path.join(d, "gt", f"f{i:03d}.png"), compress_level=1)
        for how in ("gt", "dists") * 3:
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "gt" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu", "--gt", os.path.join(d, "gt")] + flags
            if how == "dists":
                cmd += ["--dists_model", os.path.join(d, "dists.npz")]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                raise SystemExit(1)   # nothing more is started on the GPU behind a failed run
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ", "dists: ")))
            say(f"{'--gt --dists_model' if how == 'dists' else '--gt alone        '} ({'this tree' if root == ROOT else 'the parent commit, built'}): {c['files_per_s']:.2f} files/s overall, "
                f"{c['steady_files_per_s']:.2f} after the first result, results left the GPU at {c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["steady_files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lo, hi = min(rates["gt"]), max(rates["gt"])
    say(f"steady files/s: --gt --dists_model {rates['dists']}, --gt alone {rates['gt']} (its own spread: {100 * (hi / lo - 1):.1f} %); the median run with DISTS is "
        f"{100 * (statistics.median(rates['dists']) / statistics.median(rates['gt']) - 1):+.1f} % against the median run without - the flag is opt-in and pays for "
        f"thirteen full-size convolutions per file")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step_repeats", type=int, default=3)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --dists_model (default: this tree)")
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
    fd, log = tempfile.mkstemp(prefix="ir_dists_bench_", suffix=".txt")
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
