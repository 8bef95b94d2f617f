#!/usr/bin/env python3
"""The centre crop on the device (--center_crop gpu: ir_resample_u8 with BOX plans, ir_resample_u8_window) measured against center_crop_arr on
the host, in the same tree:

  1. HIP-event time per file of the whole crop chain (resample.ResizeSlot.to_network on a crop geometry: the BOX halvings, the final bicubic as a
     window call into the network input) for 2040 x 1356 -> 512 x 512 and 6000 x 4000 -> 512 x 512, with warm-up and `--repeats` timed event pairs
     of BATCH files each; center_crop_arr's host time for the same files (one thread); every device crop is compared with the host's before it is
     timed.
  2. The crop's share of the eval_batch.py step: events around ir_pipeline alone for a batch of four 512 x 512 images in the same process.
  3. files/s of eval_batch.py (a child process over K synthetic 2040 x 1356 JPEGs) alternating --center_crop host, gpu, and gpu with
     --jpeg_decoder gpu, three runs each way, at the default --workers and at --workers 2. A run's rate is its files over its wall time less the
     wall time of a run over one batch (start-up: the models' load; the median of three such runs). The host runs are the behaviour of before the flag; their spread is the allowance.

    python tools/bench_center_crop.py [--files 192] [--repeats 20] [--skip_cli] [--out profiles/center_crop.txt]
"""
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

BATCH = 4
SIZE = 512
FILES = [(2040, 1356), (6000, 4000)]   # (w, h): a DIV2K validation file, a 24-Mpixel camera file


def photo(w, h, seed):
    """Low-passed noise over a gradient: content a JPEG codes at a photograph's rate."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    from PIL import Image
    img = np.asarray(Image.fromarray(small).resize((w, h), Image.BICUBIC)).astype(np.int16)
    img += rng.integers(-12, 13, (h, w, 3), dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def device_leg(a):
    import torch
    from PIL import Image
    import bench
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    from instarevive_amd.resample import ResizeJob, ResizeSlot, chain_ws_bytes, crop_geometry
    from instarevive_amd.utils import center_crop_arr
    device = torch.device("cuda", 0)
    swin, vae, dit, sched, sds = bench.build_models(device, say)
    y, mask = bench.synthetic_prompt()
    ctx = dit.ctx
    st = _Staging.get(ctx, BATCH, SIZE, SIZE)
    st.fill(0, [photo(SIZE, SIZE, k) for k in range(BATCH)])
    st.upload(0)
    _prepare_fused(dit, y.to(device), mask.to(device), SIZE, SIZE, False, 512, (vae, swin))
    flags = _pipeline_flags(dit, "none", False, False)
    acp, sf = float(sched.alphas_cumprod[400]), float(vae.config.scaling_factor)
    step_ms = []
    for i in range(a.step_repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _launch_pipeline(ctx, st, 0, BATCH, SIZE, SIZE, flags, 512, 448, acp, sf, True)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            step_ms.append(e0.elapsed_time(e1))
    step = statistics.median(step_ms)
    say(f"eval_batch.py step, {BATCH} images of {SIZE} x {SIZE} (ir_pipeline alone, with stage-1 output, input resident on the device): {spread(step_ms)}")
    for w, h in FILES:
        img = photo(w, h, w)
        geo = crop_geometry((w, h), 1, SIZE)
        records = [ResizeJob(img, geo)] * BATCH
        host_ms = []
        for _ in range(max(a.repeats // 4, 3)):
            t0 = time.perf_counter()
            want = center_crop_arr(Image.fromarray(img), SIZE)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        rs = ResizeSlot(ctx)
        rs.fill(records)
        rs.upload()
        ctx.workspace(max(chain_ws_bytes(records), 1))
        d_in = torch.empty((BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device=device)
        for _ in range(3):
            rs.to_network(records, d_in)
        torch.cuda.synchronize()
        assert all(np.array_equal(d_in[k].cpu().numpy(), want) for k in range(BATCH)), (w, h)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rs.to_network(records, d_in)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / BATCH)
        med = statistics.median(ms)
        steps = " -> ".join(f"{tw} x {th}" for tw, th in ((w, h),) + geo.chain)
        say(f"crop chain {steps}, window at {geo.crop} (per file of {BATCH} per event pair, launches included, the same decoded file {BATCH} times so part of it stays in the last-level cache; equal to center_crop_arr): {spread(ms)}; "
            f"a batch of {BATCH} is {100 * BATCH * med / step:.2f} % of the step's {step:.2f} ms")
        say(f"center_crop_arr on the host, the same file (one thread, decoded already): {spread(host_ms)} = {statistics.median(host_ms) / med:.0f} x the device's time")
    return sds


def cli_leg(a, sds):
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_center_crop_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        w, h = FILES[0]
        for name, count in (("few", BATCH), ("in", a.files)):
            os.makedirs(os.path.join(d, name))
            for k in range(count):   # sixteen different images, repeated under new names
                src = os.path.join(d, "in", f"f{k % 16:03d}.jpg")
                if name == "in" and k >= 16:
                    shutil.copyfile(src, os.path.join(d, name, f"f{k:03d}.jpg"))
                else:
                    Image.fromarray(photo(w, h, 100 + k)).save(os.path.join(d, name, f"f{k:03d}.jpg"), quality=92)
        # gpu: the device crops what PIL decoded; gpu+dec: it decodes the JPEG as well, and only compressed bytes are uploaded
        ways = {"host": ["--center_crop", "host"], "gpu": ["--center_crop", "gpu"], "gpu+dec": ["--center_crop", "gpu", "--jpeg_decoder", "gpu"]}

        def run(folder, how, workers):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            shutil.rmtree(out + "-cond", ignore_errors=True)
            cmd = [sys.executable, os.path.join(ROOT, "eval_batch.py"), "--input", os.path.join(d, folder), "--output", out, "--batch_size", str(BATCH),
                   "--workers", str(workers), "--png_encoder", "gpu"] + ways[how] + flags
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
            dt = time.perf_counter() - t0
            written = len(os.listdir(out)) if os.path.isdir(out) else 0
            if r.returncode:
                say(f"--center_crop {how} --workers {workers} on {folder}: FAILED (rc {r.returncode}, {written} files) {r.stderr[-400:]}")
                return None
            return dt

        for workers in (-1, 2):
            start = {}
            for how in ways:   # start-up (the models' load, the first batch): the median of three runs over one batch
                few = [t for t in (run("few", how, workers) for _ in range(3)) if t is not None]
                start[how] = statistics.median(few) if few else None
            for how in tuple(ways) * 3:
                dt = run("in", how, workers)
                if dt is None or start[how] is None:
                    continue
                rate = (a.files - BATCH) / (dt - start[how])
                say(f"--center_crop {how:7s} --workers {workers:2d}: {a.files} files in {dt:.2f} s, {BATCH} files in {start[how]:.2f} s (median of three): {rate:.2f} files/s beyond start-up")
                rates.setdefault((how, workers), []).append(rate)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for workers in (-1, 2):
        host = rates.get(("host", workers))
        for how in ("gpu", "gpu+dec"):
            gpu = rates.get((how, workers))
            if host and gpu:
                allow = max(host) - min(host)
                say(f"at --workers {workers}: --center_crop {how} {[round(v, 2) for v in gpu]} files/s, --center_crop host {[round(v, 2) for v in host]}; the host runs spread over "
                    f"{allow:.2f} files/s (the allowance); the median {how} run is {100 * (statistics.median(gpu) / statistics.median(host) - 1):+.1f} % of the median host run, "
                    f"the lowest {how} run is {'not below' if min(gpu) >= min(host) - allow else 'BELOW'} the lowest host run less the allowance")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    try:
        sds = device_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds)
        else:
            say("eval_batch.py files/s: not measured in this run (--skip_cli)")
    finally:
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
