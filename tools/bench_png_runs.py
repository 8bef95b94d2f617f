#!/usr/bin/env python3
"""The run mode of the device PNG encoder (ir_png_encode_runs, --png_encoder gpu --png_runs) measured against the default mode of the same
library (ir_png_encode) in the same process:

  1. HIP-event time per 2048 x 2048 result of both entry points, ALTERNATING (one timed event pair of BATCH calls of the one, then of the
     other, `--repeats` times), over rotating device copies of the input that together exceed the last-level cache, after warm-up; on a
     restored-photograph-like image (tests/support/png_model.synthetic_b enlarged to 2048 x 2048) and on a half-flat one (its top half a
     constant colour). Every stream is decoded and compared with the filtered bytes before it is timed. Next to the network step (events around
     ir_pipeline alone) measured in the same process: the run mode's share of the step and its ratio to the default mode.
  2. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu as a child process over K synthetic 512 x 512 PNGs) without and
     with --png_runs, three runs each, alternating.

    python tools/bench_png_runs.py [--files 16] [--repeats 20] [--skip_cli] [--out FILE]"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

EDGE = 2048
BATCH = 8
LAST_LEVEL_CACHE = 256 << 20


def _images():
    from PIL import Image
    from tests.support import png_model as M
    photo = np.array(Image.fromarray(M.synthetic_b()).resize((EDGE, EDGE), Image.BICUBIC))
    half = photo.copy()
    half[:EDGE // 2] = (96, 144, 208)
    return [("restored-photograph-like (png_model.synthetic_b, bicubic to 2048 x 2048)", photo), ("half flat (its top half one colour)", half)]


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    from tests.support import png_model as M
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
    rotate = max(2, -(-LAST_LEVEL_CACHE // (3 * EDGE * EDGE)) + 1)
    stride = (int(ctx.lib.ir_png_bound(EDGE, EDGE)) + 255) & ~255
    out = torch.empty((1, stride), dtype=torch.uint8, device=device)
    info = torch.zeros(1, dtype=torch.int32, device=device)
    modes = {"ir_png_encode": L.STAGE_PNG, "ir_png_encode_runs": L.STAGE_PNG_RUNS}
    ws = {name: torch.empty(ctx.ws_bytes(stage, 1, EDGE, EDGE), dtype=torch.uint8, device=device) for name, stage in modes.items()}
    say(f"workspace: ir_png_encode {ws['ir_png_encode'].numel()} bytes, ir_png_encode_runs {ws['ir_png_encode_runs'].numel()}")
    for title, img in _images():
        filtered = M.paeth_filter(img).tobytes()
        ins = [torch.from_numpy(img).to(device)[None].contiguous() for _ in range(rotate)]
        nth = [0]

        def call(name):
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(getattr(ctx.lib, name)(ctx.h, ctx.stream(), L.ptr(ins[k]), 1, EDGE, EDGE, 3 * EDGE, EDGE, EDGE, L.ptr(out), stride, L.ptr(info),
                                             L.ptr(ws[name]), ws[name].numel()), name)
        size = {}
        for name in modes:
            for _ in range(3):
                call(name)
            torch.cuda.synchronize()
            size[name] = int(info[0])
            assert zlib.decompress(out[0, :size[name]].cpu().numpy().tobytes()) == filtered, f"{name}: the stream does not decode to the filtered rows"
        ms = {name: [] for name in modes}
        for _ in range(a.repeats):
            for name in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BATCH):
                    call(name)
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / BATCH)
        say(title + f" ({rotate} rotating inputs, per call of {BATCH} per event pair, the two entry points alternating):")
        for name in modes:
            med = statistics.median(ms[name])
            say(f"    {name}: {spread(ms[name])}; {100 * med / step:.3f} % of the step's {step:.2f} ms; {size[name]} bytes")
        lit, runs = (statistics.median(ms[name]) for name in modes)
        say(f"    run mode / default mode: {runs / lit:.2f} in time, {size['ir_png_encode_runs'] / size['ir_png_encode']:.3f} in bytes; the run mode is "
            + ("within" if runs <= 0.01 * step else "ABOVE") + " 1 % of the step")
        del ins
    return sds


def cli_leg(a, sds):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_png_runs_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        legs = [("--png_encoder gpu", []), ("--png_encoder gpu --png_runs", ["--png_runs"])]
        for _ in range(3):
            for name, extra in legs:
                out = os.path.join(d, "out")
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4",
                       "--png_encoder", "gpu"] + extra + flags
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
                rate = A.parse_cli_rate(r.stdout)
                files = [os.path.join(out, f) for f in os.listdir(out) if f.endswith(".png")] if os.path.isdir(out) else []
                if r.returncode or not rate or len(files) != a.files:
                    say(f"{name}: FAILED (rc {r.returncode}, {len(files)} of {a.files} files) {r.stderr[-400:]}")
                    continue
                c = rate[0]
                say(f"{name}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                    f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads, {sum(map(os.path.getsize, files)) / len(files) / 1e6:.2f} MB per file)")
                rates.setdefault(name, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lit, runs = (rates.get(name) for name, _ in legs)
    if lit and runs:
        say(f"files/s without the flag {[round(v, 3) for v in lit]}, with it {[round(v, 3) for v in runs]}; medians {statistics.median(lit):.3f} and "
            f"{statistics.median(runs):.3f}, the default mode's own spread {max(lit) - min(lit):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
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
