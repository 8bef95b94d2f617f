#!/usr/bin/env python3
"""The device PNG decoder (ir_png_decode, --png_decoder gpu) measured against the host decoder of the same tree (PIL):

  1. HIP-event time of ir_png_decode per file, with warm-up and `--repeats` timed event pairs of BATCH calls, for photograph-like 2048 x 2048
     and 512 x 512 files at Pillow's default level and at level 1, next to Pillow's decode and PngSource.open on one host core, the bytes
     uploaded either way and the share of the 2048 x 2048 network step; for the 2048 x 2048 default-level file also at every --span_bits
     value (png_decode.SPAN_BITS is chosen from this line). Every result is compared with Pillow's pixels first.
  2. The split by phase: the same calls in a child process under `rocprofv3 --kernel-trace --stats`, its per-kernel averages summed per phase.
  3. The command line over `--files` 2048 x 2048 PNGs (--degrade lq, the full-size input is what is decoded; --png_encoder gpu), three runs
     each: --png_decoder host and gpu at --workers 14 and 2. The host runs' own spread is the allowance for calling two rates different.

    python tools/bench_png_decode.py [--files 8] [--repeats 20] [--skip_step] [--skip_phases] [--skip_cli] [--out FILE]"""
import argparse
import csv
import glob
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

from tools.bench_jpeg import _image  # noqa: E402  (the photograph-like content of the encoders' measurements)
from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

EDGE = 2048
BATCH = 4
PHASES = (("find", ("png_find",)), ("size", ("png_walk_kernel<false>", "png_walk_kernel<0>")), ("chain", ("png_chain",)),
          ("write", ("png_walk_kernel<true>", "png_walk_kernel<1>")), ("resolve", ("png_round", "png_gather")), ("adler", ("png_adler",)),
          ("unfilter", ("png_unfilter",)), ("rgb", ("png_rgb",)))


def _pil_file(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", **kw)
    return b.getvalue()


def _pil_decode(data):
    from PIL import Image
    t0 = time.perf_counter()
    px = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
    return px, time.perf_counter() - t0


def bench_files():
    """[(name, file bytes)] in the order of the report."""
    return [(f"{e} x {e} {name}", _pil_file(_image(e, e), **kw)) for e in (EDGE, 512) for name, kw in (("default level", {}), ("level 1", dict(compress_level=1)))]


def _staged(ctx, src):
    import torch
    host = torch.zeros((src.blob_bytes + 255) & ~255, dtype=torch.uint8)
    src.pack(host.numpy(), 0)
    dev = host.to(ctx.device)
    out = torch.empty((src.h, 3 * src.w), dtype=torch.uint8, device=ctx.device)
    info = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    return dev, out, info, src.record(dev.data_ptr(), out.data_ptr())


def kernel_leg(a):
    import torch
    from instarevive_amd import png_decode as P
    step = sds = ctx = None
    if not a.skip_step:
        from tools.bench_jpeg_decode import step_ms_of
        step, sds, ctx = step_ms_of(a)
    if ctx is None:
        from instarevive_amd.models import get_context
        ctx = get_context(torch.device("cuda", 0))
    for name, data in bench_files():
        src, why = P.PngSource.open(data)
        assert src is not None, why
        want, _ = _pil_decode(data)
        host_s = min(_pil_decode(data)[1] for _ in range(3))
        t0 = time.perf_counter()
        for _ in range(3):
            P.PngSource.open(data)
        open_s = (time.perf_counter() - t0) / 3
        dev, out, info, rec = _staged(ctx, src)
        sweep = [P.SPAN_BITS] + ([b for b in a.span_bits if b != P.SPAN_BITS] if name == f"{EDGE} x {EDGE} default level" else [])
        for bits in sweep:
            ws = torch.empty(P.ws_bytes([src], bits), dtype=torch.uint8, device=ctx.device)
            for _ in range(2):
                P.launch(ctx, [rec], info.data_ptr(), bits, ws=ws)
            torch.cuda.synchronize()
            assert int(info[0]) == 0 and np.array_equal(out.cpu().numpy().reshape(want.shape), want), "the pixels differ from Pillow's"
            t = P.tables(ws.cpu().numpy(), src, bits)
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BATCH):
                    P.launch(ctx, [rec], info.data_ptr(), bits, ws=ws)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / BATCH)
            med = statistics.median(ms)
            share = f"; {100 * med / step:.3f} % of the {EDGE} x {EDGE} step's {step:.2f} ms" if step and name.startswith(str(EDGE)) else ""
            say(f"ir_png_decode {name}, span_bits {bits} (per call of {BATCH} per event pair; the pixels equal Pillow's): {spread(ms)}{share}; "
                f"{len(t['chain'])} chain entries of {int((t['cand'] != P.NONE).sum())} candidates, {int(t['flags'].sum())} squaring rounds changed something; "
                f"Pillow on one host core {1e3 * host_s:.2f} ms, PngSource.open {1e3 * open_s:.2f} ms; {src.blob_bytes} bytes uploaded against "
                f"{src.size} decoded ({100 * src.blob_bytes / src.size:.1f} %); workspace {ws.numel() / 2**20:.1f} MiB")
            del ws
    return sds


def phase_child(a):
    """What the profiler watches: `--repeats` calls per file, nothing else on the device."""
    import torch
    from instarevive_amd import png_decode as P
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    name, data = bench_files()[a.phase_child]
    src, _ = P.PngSource.open(data)
    dev, out, info, rec = _staged(ctx, src)
    ws = torch.empty(P.ws_bytes([src]), dtype=torch.uint8, device=ctx.device)
    for _ in range(a.repeats):
        P.launch(ctx, [rec], info.data_ptr(), ws=ws)
    torch.cuda.synchronize()
    assert int(info[0]) == 0


def phase_leg(a):
    for k, (name, _) in enumerate(bench_files()):
        if "level 1" in name:
            continue
        d = tempfile.mkdtemp(prefix="ir_png_decode_prof_")
        try:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ks", "--", sys.executable, os.path.abspath(__file__),
                   "--phase_child", str(k), "--repeats", str(a.repeats)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
            found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if r.returncode or not found:
                say(f"phases of {name}: the profiler run failed (rc {r.returncode}) {r.stderr[-300:]}")
                continue
            per = {}
            for row in csv.DictReader(open(found[0])):
                kname, total = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
                for phase, keys in PHASES:
                    if any(key in kname for key in keys):
                        per[phase] = per.get(phase, 0.0) + total / a.repeats / 1e6
                        break
            say(f"phases of {name} at the product's span_bits (kernel time per call, rocprofv3 --kernel-trace --stats over {a.repeats} calls): "
                + ", ".join(f"{phase} {per.get(phase, 0.0):.3f} ms" for phase, _ in PHASES) + f"; sum {sum(per.values()):.3f} ms")
        finally:
            shutil.rmtree(d, ignore_errors=True)


def cli_leg(a, sds):
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_png_decode_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        os.makedirs(os.path.join(d, "in"))
        for i in range(a.files):
            Image.fromarray(_image(EDGE, 900 + i)).save(os.path.join(d, "in", f"f{i:03d}.png"))
        common = ["--degrade", "lq", "--png_encoder", "gpu"]
        for workers in ("14", "2"):
            for dec in ("host", "gpu"):
                name = f"--png_decoder {dec} --workers {workers}"
                for _ in range(3):
                    out = os.path.join(d, "out")
                    shutil.rmtree(out, ignore_errors=True)
                    cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--input", os.path.join(d, "in"), "--output", out] + common + \
                          ["--png_decoder", dec, "--workers", workers] + flags
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
                    rate = A.parse_cli_rate(r.stdout)
                    written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
                    if r.returncode or not rate or written != a.files:
                        say(f"{name}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                        continue
                    c = rate[0]
                    note = " ".join(ln.split("] ", 1)[-1] for ln in r.stdout.splitlines() if "--png_decoder gpu:" in ln and "decoded on the device" in ln)
                    say(f"{name}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                        f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {note}")
                    rates.setdefault(name, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for workers in ("14", "2"):
        host, gpu = (rates.get(f"--png_decoder {dec} --workers {workers}") for dec in ("host", "gpu"))
        if host and gpu:
            allowance = max(host) - min(host)
            diff = statistics.median(gpu) - statistics.median(host)
            say(f"--workers {workers}: device decoder {[round(v, 3) for v in gpu]} files/s, host decoder {[round(v, 3) for v in host]} (its own spread "
                f"{allowance:.3f} is the allowance); medians differ by {diff:+.3f}: "
                + ("inside the allowance, no difference shown" if abs(diff) <= allowance else "OUTSIDE the allowance"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--span_bits", type=int, nargs="*", default=[4096, 16384, 65536, 262144, 1048576], help="span sizes timed on the 2048 x 2048 default-level file")
    ap.add_argument("--skip_step", action="store_true", help="do not build the models for the share of the network step")
    ap.add_argument("--skip_phases", action="store_true")
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--phase_child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if a.phase_child is not None:
        return phase_child(a)
    try:
        sds = kernel_leg(a)
        if not a.skip_phases:
            phase_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds)
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
