#!/usr/bin/env python3
"""The device JPEG decoder (ir_jpeg_decode, --jpeg_decoder gpu) measured against the host decoder of the same tree (PIL):

  1. HIP-event time of ir_jpeg_decode per file, with warm-up and `--repeats` timed event pairs of BATCH calls, for the photograph fixture
     (tests/golden/jpeg_photo_640x419.jpg), Pillow-encoded quality-95 4:2:0 files of 512 x 512 and 2048 x 2048 (photograph-like content) and the
     96 x 272 quality-100 noise file whose stream hardly synchronises; the bytes uploaded against the decoded image; the 2048 x 2048 file at
     subseq_bits 256 / 512 / 1024 / 2048 (jpeg_decode.SUBSEQ_BITS is chosen from this line). Every result is compared with Pillow's pixels
     before it is timed.
  2. Pillow's decode of the same files on one host core.
  3. The share of the 2048 x 2048 network step (events around ir_pipeline alone) measured in the same process (--skip_step leaves it out).
  4. files/s of the command line (inference.py as a child process over K 2048 x 2048 JPEG ground-truth files, --degrade lq --save_format jpg
     --jpeg_encoder gpu), three runs each: --jpeg_decoder host on --baseline_root (a built checkout of the parent commit, without the flag;
     default: this tree with --jpeg_decoder host), whose run-to-run spread is the allowance for calling two rates different, then
     --jpeg_decoder gpu and host at --workers 2 and 14.

    python tools/bench_jpeg_decode.py [--files 8] [--repeats 20] [--skip_step] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
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

from tools.bench_jpeg import _image  # noqa: E402  (the photograph-like content of the encoder's measurement)
from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

EDGE = 2048
BATCH = 8
PHOTO = os.path.join(ROOT, "tests", "golden", "jpeg_photo_640x419.jpg")


def _pil_file(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", **kw)
    return b.getvalue()


def _pil_decode(data):
    from PIL import Image
    t0 = time.perf_counter()
    px = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
    return px, time.perf_counter() - t0


def bench_files():
    """[(name, file bytes)] in the order of the report."""
    rng = np.random.default_rng(5)
    return [("photograph 640 x 419 (the fixture)", open(PHOTO, "rb").read()),
            ("512 x 512 quality 95 4:2:0", _pil_file(_image(512, 512), quality=95, subsampling=2)),
            ("2048 x 2048 quality 95 4:2:0", _pil_file(_image(EDGE, EDGE), quality=95, subsampling=2)),
            ("96 x 272 noise quality 100 4:4:4", _pil_file(rng.integers(0, 256, (96, 272, 3), dtype=np.uint8), quality=100, subsampling=0))]


def step_ms_of(a):
    import torch
    import bench
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
    ms = []
    for i in range(a.step_repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _launch_pipeline(ctx, st, 0, 1, EDGE, EDGE, flags, 512, 448, acp, sf, False)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    say(f"network step at {EDGE} x {EDGE} (ir_pipeline alone, input resident on the device): {spread(ms)}")
    return statistics.median(ms), sds, ctx


def kernel_leg(a):
    import torch
    from instarevive_amd import jpeg_decode as J
    step, sds, ctx = (None, None, None) if a.skip_step else step_ms_of(a)
    if ctx is None:
        from instarevive_amd.models import get_context
        ctx = get_context(torch.device("cuda", 0))
    for name, data in bench_files():
        src, why = J.JpegSource.open(data)
        assert src is not None, why
        want, _ = _pil_decode(data)
        host_s = min(_pil_decode(data)[1] for _ in range(3))
        t0 = time.perf_counter()
        for _ in range(3):
            J.JpegSource.open(data)
        parse_s = (time.perf_counter() - t0) / 3
        host = torch.zeros((src.blob_bytes + 255) & ~255, dtype=torch.uint8)
        src.pack(host.numpy(), 0)
        dev = host.to(ctx.device)
        out = torch.empty((src.plan.h, 3 * src.plan.w), dtype=torch.uint8, device=ctx.device)
        info = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        rec = src.record(dev.data_ptr(), out.data_ptr())
        for bits in ([J.SUBSEQ_BITS] + [b for b in a.subseq_bits if b != J.SUBSEQ_BITS] if "2048 x 2048" in name else [J.SUBSEQ_BITS]):
            ws = torch.empty(J.ws_bytes([src], bits), dtype=torch.uint8, device=ctx.device)
            for _ in range(3):
                J.launch(ctx, [rec], info.data_ptr(), bits, ws=ws)
            torch.cuda.synchronize()
            assert int(info[0]) == 0 and np.array_equal(out.cpu().numpy().reshape(want.shape), want), "the pixels differ from Pillow's"
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(BATCH):
                    J.launch(ctx, [rec], info.data_ptr(), bits, ws=ws)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / BATCH)
            med = statistics.median(ms)
            share = f"; {100 * med / step:.3f} % of the {EDGE} x {EDGE} step's {step:.2f} ms" if step and "2048 x 2048" in name else ""
            say(f"ir_jpeg_decode {name}, subseq_bits {bits} (per call of {BATCH} per event pair; the pixels equal Pillow's): {spread(ms)}{share}; "
                f"Pillow on one host core {1e3 * host_s:.2f} ms, the host's parse and byte pass {1e3 * parse_s:.2f} ms; {src.blob_bytes} bytes uploaded against "
                f"{src.size} decoded ({100 * src.blob_bytes / src.size:.1f} %); workspace {ws.numel() / 2**20:.1f} MiB")
            del ws
    return sds


def cli_leg(a, sds):
    from PIL import Image
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_jpeg_decode_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        os.makedirs(os.path.join(d, "in"))
        for i in range(a.files):
            Image.fromarray(_image(EDGE, 900 + i)).save(os.path.join(d, "in", f"f{i:03d}.jpg"), quality=95, subsampling=2)
        common = ["--degrade", "lq", "--save_format", "jpg", "--jpeg_encoder", "gpu"]
        base_name = "parent commit, host decoder, --workers 14"
        legs = [(base_name, a.baseline_root or ROOT, common + ["--workers", "14"] + ([] if a.baseline_root else ["--jpeg_decoder", "host"]))]
        for workers in ("14", "2"):
            for dec in ("host", "gpu"):
                legs.append((f"--jpeg_decoder {dec} --workers {workers}", ROOT, common + ["--jpeg_decoder", dec, "--workers", workers]))
        for name, root, extra in legs:
            for _ in range(3):
                out = os.path.join(d, "out")
                shutil.rmtree(out, ignore_errors=True)
                cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out] + extra + flags
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
                rate = A.parse_cli_rate(r.stdout)
                written = len([f for f in os.listdir(out) if f.endswith(".jpg")]) if os.path.isdir(out) else 0
                if r.returncode or not rate or written != a.files:
                    say(f"{name}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                    continue
                c = rate[0]
                note = " ".join(ln.split("] ", 1)[-1] for ln in r.stdout.splitlines() if "--jpeg_decoder gpu:" in ln and "decoded on the device" in ln)
                say(f"{name}: {c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                    f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {note}")
                rates.setdefault(name, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    base = rates.get(base_name)
    if base:
        allowance = max(base) - min(base)
        say(f"the baseline's own spread is {allowance:.3f} files/s ({100 * allowance / statistics.median(base):.1f} %): the allowance for calling two rates different")
        for workers in ("14", "2"):
            host, gpu = (rates.get(f"--jpeg_decoder {dec} --workers {workers}") for dec in ("host", "gpu"))
            if host and gpu:
                diff = statistics.median(gpu) - statistics.median(host)
                say(f"--workers {workers}: device decoder {[round(v, 3) for v in gpu]} files/s, host decoder {[round(v, 3) for v in host]}; medians differ by "
                    f"{diff:+.3f}: " + ("inside the allowance, no difference shown" if abs(diff) <= allowance else "OUTSIDE the allowance"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--subseq_bits", type=int, nargs="*", default=[256, 512, 1024, 2048], help="subsequence sizes timed on the 2048 x 2048 file")
    ap.add_argument("--skip_step", action="store_true", help="do not build the models for the share of the network step")
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the baseline runs (default: this tree, --jpeg_decoder host)")
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
