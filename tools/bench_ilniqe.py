#!/usr/bin/env python3
"""The device part of IL-NIQE (ir_ilniqe_stats, --ilniqe_params) measured against the host model of the same tree (tools/evaluate_ilniqe.py):

  1. HIP-event time of ir_ilniqe_stats per image for K seeded images of 512 x 512 and of 2048 x 2048 (every size costs the same 504 x 504
     evaluation behind the resize), with warm-up, `--repeats` timed event pairs of BATCH calls over rotating inputs. Every result is compared
     with the host model before it is timed (plane 0 and the mean / variance bit-equal, counts equal).
  2. The split: the kernels' own durations from one traced call (torch.profiler's device activity, grouped by kernel name) - resize (the two
     resize passes, the opponent planes, the 6 x 6 down-filter), DFT (the matrix products), derivatives, statistics (MSCN, the log planes and
     every block kernel, Weibull fits included) - and the DFT's achieved share of the fp64 matrix peak (--peak_tflops, default 78.6: the
     MI355X's published fp64 matrix rate) from its 2 x 8 N^3 (4 N^3 for the real forward pass) flop per transform.
  3. The host model's seconds per image on the same files (numpy / scipy fp64) and the host part that stays on the host (fits + score).
  4. bench.py's headline step time without the flag is recorded next to it by running `python bench.py --gpus 1 --steps K --warmup W`.

    python tools/bench_ilniqe.py [--images 4] [--repeats 20] [--peak_tflops 78.6] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)

BATCH = 4
GROUPS = {"resize": ("resize_cols", "resize_rows", "down6"), "DFT": ("dft_gemm",), "derivatives": ("deriv_kernel",),
          "statistics": ("mscn_kernel", "mscn_fields", "log_mean", "log_planes", "aggd_kernel", "mean_var", "weibull")}


def _image(edge, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 6.0, base.shape)), 1, 254).astype(np.uint8)


def dft_flop() -> float:
    """Per image: per scale one real forward transform (4 N^3 + 8 N^3) and twelve complex inverse transforms (2 x 8 N^3)."""
    return sum((12.0 + 12 * 16.0) * n ** 3 for n in (504, 252))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--peak_tflops", type=float, default=78.6)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    import torch
    import evaluate_ilniqe as EI
    from instarevive_amd import _lib as L, ilniqe
    try:
        ctx = L.Context(0)
        t0 = time.perf_counter()
        ilniqe.configure(ctx)
        say(f"ilniqe.configure (tables in numpy fp64, 42 MB uploaded, twiddles made by the library): {time.perf_counter() - t0:.2f} s, once per run")
        rng = np.random.default_rng(1)
        d = 40
        par = (rng.normal(size=d), np.eye(d), rng.normal(size=468), np.linalg.qr(rng.normal(size=(468, d)))[0])
        for edge in (512, 2048):
            imgs = [_image(edge, 10 * edge + i) for i in range(a.images)]
            host_s, part_s = [], []
            for img in imgs:
                t0 = time.perf_counter()
                want = EI.image_stats(img)
                t1 = time.perf_counter()
                EI.score_features(EI.features_from_stats(want), par)
                host_s.append(time.perf_counter() - t0)
                got = ilniqe.stats_arrays(ctx, img)
                assert np.array_equal(got[:, :, :30], want[:, :, :30]) and np.array_equal(got[:, :, 498:504], want[:, :, 498:504]), "plane 0 / mean-variance differ from the host model"
                t0 = time.perf_counter()
                ilniqe.score(ilniqe.features_from_stats(got), par)
                part_s.append(time.perf_counter() - t0)
            say(f"host model (tools/evaluate_ilniqe.py, numpy / scipy fp64) on {a.images} images of {edge} x {edge}: {statistics.median(host_s):.2f} s per image "
                f"(min {min(host_s):.2f}, max {max(host_s):.2f}); the part that stays on the host (fits + score) {1e3 * statistics.median(part_s):.1f} ms per image")
            dev = [torch.from_numpy(i).to(ctx.device) for i in imgs]
            out = torch.zeros((ilniqe.ROW,), dtype=torch.float64, device=ctx.device)
            nth = [0]

            def call():
                t = dev[nth[0] % len(dev)]
                nth[0] += 1
                ilniqe.queue_stats(ctx, t.data_ptr(), edge, 3 * edge, 1, edge, edge, out)
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
            say(f"ir_ilniqe_stats {edge} x {edge}, n = 1 ({len(dev)} rotating inputs, per call of {BATCH} per event pair; plane 0 and mean / variance bit-equal to the "
                f"host model): {spread(ms)} per image; the host model takes {1e3 * statistics.median(host_s) / statistics.median(ms):.0f} times as long")
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    call()
                    torch.cuda.synchronize()
                split = {g: 0.0 for g in GROUPS}
                other = 0.0
                for ev in prof.key_averages():
                    us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    hit = [g for g, keys in GROUPS.items() if any(k in ev.key for k in keys)]
                    if hit:
                        split[hit[0]] += us / 1e3
                    else:
                        other += us / 1e3
                say(f"  one traced call, kernel durations by name: " + ", ".join(f"{g} {v:.3f} ms" for g, v in split.items()) + f" (other device activity {other:.3f} ms)")
                if split["DFT"] > 0:
                    rate = dft_flop() / (split["DFT"] * 1e-3) / 1e12
                    say(f"  DFT: {dft_flop() / 1e9:.1f} GFLOP of fp64 matrix products per image in {split['DFT']:.3f} ms = {rate:.1f} TFLOP/s, "
                        f"{100 * rate / a.peak_tflops:.1f} % of the {a.peak_tflops} TFLOP/s fp64 matrix peak")
            except Exception as e:   # the split needs a torch whose profiler sees HIP kernels; the totals above do not
                say(f"  no split: torch.profiler gave no device activity ({type(e).__name__}: {e})")
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
