#!/usr/bin/env python3
"""The device JPEG encoder (ir_jpeg_encode, --save_format jpg --jpeg_encoder gpu) measured against the host encoder of the same tree (PIL):

  1. HIP-event time of ir_jpeg_encode at quality 95 / 4:2:0 for one 2048 x 2048 result and for a batch of four 512 x 512 results on
     photograph-like content, with warm-up, `--repeats` timed event pairs of BATCH calls over rotating inputs that together exceed the
     last-level cache, next to the network step (events around ir_pipeline alone) measured in the same process. Every segment is compared
     with PIL's file before it is timed (the same bytes). The restart intervals in `--restarts` are timed on the 2048 x 2048 image:
     jpeg.RESTART_MCUS is chosen from this line.
  2. PIL's time for the same images on one host core, and the bytes that cross to the host against the raw result.
  3. files/s of the command line (inference.py --sr_scale 4 as a child process over K synthetic 512 x 512 PNGs), three runs each:
     the default PNG run on --baseline_root (a built checkout of the parent commit; default this tree), whose run-to-run spread is the
     allowance for calling two rates different, then --save_format jpg with the host and with the device encoder at --workers 14 and 2.

    python tools/bench_jpeg.py [--files 16] [--repeats 20] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
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

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

EDGE = 2048
BATCH = 8
LAST_LEVEL_CACHE = 256 << 20
SHAPES = [(2048, 1), (512, 4)]   # (edge, n)
QUALITY, SUBSAMPLING = 95, 2


def _image(edge, seed):
    """A smooth image with sigma-2 noise: what a restored photograph looks like to an entropy coder."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 2.0, base.shape)), 0, 255).astype(np.uint8)


def _pil(img, restart):
    from PIL import Image
    b = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(img).save(b, format="JPEG", quality=QUALITY, subsampling=SUBSAMPLING, restart_marker_blocks=restart)
    return b.getvalue(), time.perf_counter() - t0


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L, jpeg
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
    for edge, n in SHAPES:
        img = _image(edge, edge)
        restarts = [jpeg.RESTART_MCUS] + ([r for r in a.restarts if r != jpeg.RESTART_MCUS] if edge == EDGE else [])
        moved = 3 * edge * edge * n
        rotate = max(2, -(-LAST_LEVEL_CACHE // moved) + 1)   # the inputs in rotation exceed the last-level cache
        t = torch.from_numpy(img).to(device)
        ins = [t.expand(n, -1, -1, -1).contiguous() for _ in range(rotate)]
        for restart in restarts:
            want, _ = _pil(img, restart)
            host_s = min(_pil(img, restart)[1] for _ in range(3))
            stride = (jpeg.bound(edge, edge, SUBSAMPLING, restart) + 255) & ~255
            out = torch.empty((n, stride), dtype=torch.uint8, device=device)
            info = torch.zeros(n, dtype=torch.int32, device=device)
            ws = torch.empty(ctx.ws_bytes(L.STAGE_JPEG, n, edge, edge, SUBSAMPLING, restart), dtype=torch.uint8, device=device)
            nth = [0]

            def call():
                k = nth[0] % rotate
                nth[0] += 1
                ctx.check(ctx.lib.ir_jpeg_encode(ctx.h, ctx.stream(), L.ptr(ins[k]), n, edge, edge, 3 * edge, edge, edge, QUALITY, SUBSAMPLING, restart,
                                                 L.ptr(out), stride, L.ptr(info), L.ptr(ws), ws.numel()), "ir_jpeg_encode")
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            sizes = info.cpu().tolist()
            for i, size in enumerate(sizes):
                assert jpeg.wrap_jpeg(out[i, :size].cpu().numpy().tobytes(), edge, edge, QUALITY, SUBSAMPLING, restart) == want, "the file differs from PIL's"
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
            say(f"ir_jpeg_encode {edge} x {edge}, n = {n}, quality {QUALITY}, 4:2:0, restart interval {restart} MCUs ({rotate} rotating inputs, per call of {BATCH} "
                f"per event pair; the files equal PIL's): {spread(ms)}; per image {100 * med / n / step:.3f} % of the {EDGE} x {EDGE} step's {step:.2f} ms; "
                f"PIL on one host core {1e3 * host_s:.1f} ms per image; {sizes[0]} bytes cross to the host per image against {3 * edge * edge} raw "
                f"({100 * sizes[0] / (3 * edge * edge):.1f} %); workspace {ws.numel() / 2**20:.1f} MiB, slot {stride / 2**20:.1f} MiB per image")
            del out, ws
        del ins
    return sds


def cli_leg(a, sds):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_jpeg_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        legs = [("png (parent commit, default run)", a.baseline_root or ROOT, [], ".png")]
        for workers in ("14", "2"):
            for enc in ("host", "gpu"):
                legs.append((f"--save_format jpg --jpeg_encoder {enc} --workers {workers}", ROOT,
                             ["--save_format", "jpg", "--jpeg_encoder", enc, "--workers", workers], ".jpg"))
        for name, root, extra, ext in legs:
            for _ in range(3):
                out = os.path.join(d, "out")
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4"] + extra + flags
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
                rate = A.parse_cli_rate(r.stdout)
                written = len([f for f in os.listdir(out) if f.endswith(ext)]) if os.path.isdir(out) else 0
                if r.returncode or not rate or written != a.files:
                    say(f"{name}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                    continue
                c = rate[0]
                note = " ".join(ln.split("] ", 1)[-1] for ln in r.stdout.splitlines() if "--jpeg_encoder gpu:" in ln)
                say(f"{name}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                    f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {note}")
                rates.setdefault(name, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    base = rates.get(legs[0][0])
    if base:
        allowance = max(base) - min(base)
        say(f"the PNG baseline's own spread is {allowance:.3f} files/s ({100 * allowance / statistics.median(base):.1f} %): the allowance for calling two rates different")
        for workers in ("14", "2"):
            host, gpu = (rates.get(f"--save_format jpg --jpeg_encoder {enc} --workers {workers}") for enc in ("host", "gpu"))
            if host and gpu:
                diff = statistics.median(gpu) - statistics.median(host)
                say(f"--workers {workers}: device encoder {[round(v, 3) for v in gpu]} files/s, host encoder {[round(v, 3) for v in host]}; medians differ by "
                    f"{diff:+.3f}: " + ("inside the allowance, no difference shown" if abs(diff) <= allowance else "OUTSIDE the allowance"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--restarts", type=int, nargs="*", default=[8, 32, 64, 128], help="restart intervals timed on the 2048 x 2048 image next to jpeg.RESTART_MCUS")
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the default PNG runs (default: this tree)")
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
