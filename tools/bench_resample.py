#!/usr/bin/env python3
"""The device resampler (ir_resample_u8, --resize gpu) measured against the host resizes of the same tree:

  1. HIP-event time of ir_resample_u8 for 512 x 512 -> 2048 x 2048 bicubic (the enlargement of --sr_scale 4) and 2048 x 2048 -> 1500 x 1500 LANCZOS
     (a result resized back), with warm-up, `--repeats` timed event pairs of BATCH calls over rotating inputs and outputs that together exceed the
     last-level cache, next to the network step (events around ir_pipeline alone) measured in the same process and to the call's HBM floor (bytes
     read + written over 8 TB/s): the budget of such side work is 1 % of the step. Every result is compared with PIL's before it is timed.
  2. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu as a child process over K synthetic 512 x 512 PNGs) alternating
     --resize host and gpu on one box in one call, at --workers 2 and at the default worker count, two runs each way.

    python tools/bench_resample.py [--files 32] [--repeats 20] [--skip_cli] [--out FILE]

Per-launch times come from a rocprofv3 --kernel-trace --stats run of `tools/bench_resample.py --skip_cli --repeats 5` (resample_pass_kernel<0> is the
horizontal pass, <1> the vertical one)."""
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

from tools.bench_png import LINES, power_note, say, spread  # noqa: E402  (one report format for both side-work tools)

EDGE = 2048
BATCH = 8
LAST_LEVEL_CACHE = 256 << 20
HBM_BYTES_PER_S = 8e12
SHAPES = [("bicubic", 0, (512, 512), (2048, 2048)), ("lanczos", 1, (2048, 2048), (1500, 1500))]


def resample_leg(a, sampler_file):
    import ctypes as C
    import torch
    from PIL import Image
    import bench
    from instarevive_amd import _lib as L
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    from instarevive_amd.resample import host_plan
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
    t0 = time.time()
    rng = np.random.default_rng(7)
    for name, flt, (ih, iw), (oh, ow) in SHAPES:
        moved = 3 * (ih * iw + oh * ow)
        rotate = max(2, -(-LAST_LEVEL_CACHE // moved) + 1)   # inputs + outputs in rotation exceed the last-level cache
        img = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        want = np.array(Image.fromarray(img).resize((ow, oh), Image.BICUBIC if flt == 0 else Image.LANCZOS))
        ins = [torch.from_numpy(img).to(device) for _ in range(rotate)]
        outs = [torch.empty((oh, ow, 3), dtype=torch.uint8, device=device) for _ in range(rotate)]
        plan = host_plan(ih, iw, oh, ow, flt).to(device)
        ws = torch.empty(max(int(ctx.lib.ir_workspace_bytes(None, L.STAGE_RESAMPLE, 1, ih, ow, 0, 0, 0)), 16), dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_resample_u8(ctx.h, ctx.stream(), L.ptr(ins[k]), 1, ih, iw, 3 * iw, L.ptr(outs[k]), oh, ow, oh, ow, 3 * ow, L.ptr(plan),
                                             L.ptr(ws), ws.numel()), "ir_resample_u8")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), want), name
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
        say(f"ir_resample_u8 {name} {ih} x {iw} -> {oh} x {ow} ({rotate} rotating input / output pairs, per call of {BATCH} per event pair; equal to PIL): {spread(ms)}; "
            f"HBM floor {floor:.4f} ms ({moved / 1e6:.1f} MB over 8 TB/s) = {med / floor:.1f} x the floor; {100 * med / step:.3f} % of the step's {step:.2f} ms "
            f"(budget 1 %): {'within' if med <= 0.01 * step else 'ABOVE'}")
    say(f"resample leg: {power_note(sampler_file, t0, time.time())}")
    return sds


def cli_leg(a, sds, sampler_file):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_resample_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        for workers in (2, -1):
            for how in ("host", "gpu", "host", "gpu"):
                out = os.path.join(d, "out")
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--workers", str(workers),
                       "--png_encoder", "gpu", "--resize", how] + flags
                t0 = time.time()
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
                rate = A.parse_cli_rate(r.stdout)
                written = len(os.listdir(out)) if os.path.isdir(out) else 0
                if r.returncode or not rate or written != a.files:
                    say(f"--resize {how} --workers {workers}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                    continue
                c = rate[0]
                say(f"--resize {how:4s} --workers {workers:2d}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                    f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads; {power_note(sampler_file, t0, time.time())})")
                rates.setdefault((how, workers), []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for workers in (2, -1):
        host, gpu = rates.get(("host", workers)), rates.get(("gpu", workers))
        if host and gpu:
            low = min(host)
            say(f"at --workers {workers}: --resize gpu {gpu} files/s, --resize host {host}; the lower --resize gpu run is "
                f"{'not below' if min(gpu) >= low else 'BELOW'} the lower --resize host run ({min(gpu):.2f} against {low:.2f}, {100 * (min(gpu) / low - 1):+.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    sampler, sampler_file = None, os.path.join(tempfile.gettempdir(), f"ir_resample_power_{os.getpid()}.txt")
    try:   # a child that only reads sysfs, started before this process's first GPU call (as bench.py does)
        sampler = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "power_sampler.py"), "--out", sampler_file], stdin=subprocess.PIPE)
    except OSError:
        sampler_file = None
    try:
        sds = resample_leg(a, sampler_file)
        if not a.skip_cli:
            cli_leg(a, sds, sampler_file)
    finally:
        if sampler is not None:
            sampler.stdin.close()
            sampler.wait(timeout=10)
            if sampler_file and os.path.exists(sampler_file):
                os.remove(sampler_file)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
