#!/usr/bin/env python3
"""The device PNG encoder (ir_png_encode, --png_encoder gpu) measured against the host encoder of the same tree:

  1. HIP-event time of ir_png_encode at 2048 x 2048 on three inputs - the seeded synthetic photograph of tests/support/png_model.py scaled to size,
     uniform noise, and a real output of the pipeline on the bench's seeded weights - with warm-up, `--repeats` timed calls and their spread, next to
     the time of the network step (events around ir_pipeline alone) measured in the same process: the encoder's budget is 1 % of the step. Sizes against PIL's levels 1
     and 6 and against the CPU model of the format are printed with them.
  2. files/s of the command line (inference.py --sr_scale 4 as a child process over K synthetic 512 x 512 PNGs, bench.py's CLI leg) alternating
     --png_encoder host and gpu on one box in one call, at --workers 2 and at the default worker count, the host encoder twice at the default.

    python tools/bench_png.py [--files 32] [--repeats 20] [--skip_cli] [--out FILE]

The clock / power trace of the card (tools/power_sampler.py) is summarised per leg. Per-launch times come from a rocprofv3 --kernel-trace --stats run
of `tools/bench_png.py --skip_cli --repeats 5` (the four kernels are png_hist_kernel, png_codes_kernel, png_encode_kernel, png_compact_kernel)."""
import argparse
import io
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

EDGE = 2048
ROTATE, BATCH = 24, 8
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def spread(ms):
    return f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} over {len(ms)} calls"


def pil_size(img, level):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=level)
    return len(b.getvalue())


def power_note(sampler_file, t0, t1):
    from tools.power_sampler import summarise
    p = summarise(sampler_file, t0, t1) if sampler_file else None
    if not p:
        return "clock / power: no readable hwmon node"
    return f"gfx clock {p.get('clock_mhz')} MHz (min {p.get('clock_mhz_min')}, max {p.get('clock_mhz_max')}), socket power {p.get('power_w')} W (max {p.get('power_w_max')}), {p['samples']} samples"


def encode_leg(a, sampler_file):
    import ctypes as C
    import torch
    import bench
    from instarevive_amd import _lib as L
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    from instarevive_amd.png import wrap_png
    from tests.support import png_model as M
    device = torch.device("cuda", 0)
    swin, vae, dit, sched, sds = bench.build_models(device, say)
    y, mask = bench.synthetic_prompt()
    lq = bench.upscale_bicubic(bench.synthetic_lq(1, 512, 512, 500), 4)
    # the network step alone: events around ir_pipeline, the input already on the device (bench.py's timed region without its transfers)
    ctx, imgs = dit.ctx, [lq[0].numpy()]
    yd, md = y.to(device), mask.to(device)
    st = _Staging.get(ctx, 1, EDGE, EDGE)
    st.fill(0, imgs)
    st.upload(0)
    _prepare_fused(dit, yd, md, EDGE, EDGE, False, 512, (vae, swin))
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
    pred = [st.d_out[0][0].cpu().numpy()]
    say(f"network step at {EDGE} x {EDGE} (ir_pipeline alone, input resident on the device): {spread(step_ms)}")
    inputs = {"synthetic A (32 x 32 field x 64 bicubic, grain sigma 1)": M.synthetic(11, 32, EDGE // 32),
              "uniform noise": np.random.default_rng(7).integers(0, 256, (EDGE, EDGE, 3), dtype=np.uint8),
              "pipeline output (seeded weights)": np.ascontiguousarray(pred[0])}
    del st
    stride = int(ctx.lib.ir_png_bound(EDGE, EDGE))
    d_out = torch.empty(stride, dtype=torch.uint8, device=device)
    d_info = torch.zeros(1, dtype=torch.int32, device=device)
    ws = torch.empty(ctx.ws_bytes(L.STAGE_PNG, 1, EDGE, EDGE), dtype=torch.uint8, device=device)
    say(f"ir_png_bound = {stride} bytes, workspace {ws.numel()} bytes")
    t0 = time.time()
    worst = 0.0
    for name, img in inputs.items():
        # ROTATE device copies of the input (302 MB, beyond the 256 MB last-level cache) so that a call does not find its pixels cached by the previous
        # one; each event pair brackets BATCH calls (one call is four sub-millisecond launches)
        copies = [torch.from_numpy(img).to(device) for _ in range(1 if a.warm else ROTATE)]
        nth = [0]

        def call():
            d = copies[nth[0] % len(copies)]
            nth[0] += 1
            ctx.check(ctx.lib.ir_png_encode(ctx.h, ctx.stream(), L.ptr(d), 1, EDGE, EDGE, 3 * EDGE, EDGE, EDGE, L.ptr(d_out), stride,
                                            L.ptr(d_info), L.ptr(ws), ws.numel()), "ir_png_encode")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / BATCH)
        size = int(d_info[0])
        png = wrap_png(d_out[:size].cpu().numpy(), EDGE, EDGE)
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), img), name
        line = f"ir_png_encode, {name} ({'one resident input, warm cache' if a.warm else f'{ROTATE} rotating inputs'}, per call of {BATCH} per event pair): {spread(ms)}; {len(png)} bytes"
        if not a.no_sizes:
            l1, l6, model = pil_size(img, 1), pil_size(img, 6), len(wrap_png(M.encode(img), EDGE, EDGE))
            line += f" = {len(png) / l1:.3f} of PIL level 1 ({l1}), {len(png) / l6:.3f} of level 6 ({l6}), {len(png) / model:.4f} of the CPU model ({model})"
        say(line)
        worst = max(worst, statistics.median(ms))
    say(f"encode leg: {power_note(sampler_file, t0, time.time())}")
    step = statistics.median(step_ms)
    say(f"budget: the slowest input's median {worst:.3f} ms is {100 * worst / step:.2f} % of the step's {step:.2f} ms (budget 1 %): {'within' if worst <= 0.01 * step else 'ABOVE'}")
    return sds


def cli_leg(a, sds, sampler_file):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_png_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        for enc, workers in (("host", 2), ("gpu", 2), ("host", -1), ("gpu", -1), ("host", -1)):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--workers", str(workers),
                   "--png_encoder", enc] + flags
            t0 = time.time()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
            rate = A.parse_cli_rate(r.stdout)
            written = len(os.listdir(out)) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"--png_encoder {enc} --workers {workers}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            bytes_out = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
            note = [ln for ln in r.stdout.splitlines() if "took the host encoder" in ln or "host-bound" in ln]
            say(f"--png_encoder {enc:4s} --workers {workers:2d}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads, {bytes_out / a.files / 1e6:.2f} MB per file; {power_note(sampler_file, t0, time.time())})"
                + "".join(f"\n    {ln.strip()}" for ln in note))
            rates.setdefault((enc, workers), []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if ("host", 2) in rates and ("gpu", 2) in rates:
        say(f"at --workers 2 the GPU encoder's {rates[('gpu', 2)][0]:.2f} files/s is {'above' if rates[('gpu', 2)][0] > rates[('host', 2)][0] else 'NOT ABOVE'} the host encoder's {rates[('host', 2)][0]:.2f}")
    if ("host", -1) in rates and ("gpu", -1) in rates:
        low = min(rates[("host", -1)])
        say(f"at the default worker count the GPU encoder's {rates[('gpu', -1)][0]:.2f} files/s is {'not below' if rates[('gpu', -1)][0] >= low else 'BELOW'} the lower host-encoder run ({low:.2f} of {rates[('host', -1)]})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--warm", action="store_true", help="encode one resident input over and over (warm cache) instead of rotating over copies")
    ap.add_argument("--no_sizes", action="store_true", help="skip the PIL / CPU-model sizes (several seconds of host work per input)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    sampler, sampler_file = None, os.path.join(tempfile.gettempdir(), f"ir_png_power_{os.getpid()}.txt")
    try:   # a child that only reads sysfs, started before this process's first GPU call (as bench.py does)
        sampler = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "power_sampler.py"), "--out", sampler_file], stdin=subprocess.PIPE)
    except OSError:
        sampler_file = None
    try:
        sds = encode_leg(a, sampler_file)
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
