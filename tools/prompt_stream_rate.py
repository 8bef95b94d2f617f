#!/usr/bin/env python3
"""images/s of process_stream() with one prompt per image (each batch an (images, y, y_mask) triple, every image its own 300-token prompt) against
the fixed prompt, full-size seeded weights (bench.py's), graph=True, alternating the two forms: the cost of projecting P prompts per batch
(ir_dit_set_prompts: caption MLP + 28 layers' K / V over P * 300 rows, queued on the stream).

    python tools/prompt_stream_rate.py [--size 512] [--batch 8] [--batches 12] [--rounds 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import bench
    from instarevive_amd.pipeline import process_stream
    dev = torch.device("cuda", 0)
    swin, vae, dit, sched, _ = bench.build_models(dev, lambda m: None)
    y, mask = bench.synthetic_prompt()
    g = torch.Generator().manual_seed(5)
    imgs = [(torch.rand(a.size, a.size, 3, generator=g) * 255).to(torch.uint8).numpy() for _ in range(a.batch)]
    prompts = [(torch.randn(a.batch, y.shape[1], y.shape[2], generator=g) * 0.1, mask.expand(a.batch, -1, -1).contiguous()) for _ in range(a.batches)]
    yc, mc = y.to(dev), mask.to(dev)

    def run(per_image):
        feed = ((imgs, *prompts[j]) if per_image else imgs for j in range(a.batches))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in process_stream(dit, feed, "wavelet", False, False, 512, 448, preprocess_model=swin, vae=vae, y=yc, y_mask=mc, noise_scheduler=sched,
                                return_stage1=False, graph=True):
            pass
        torch.cuda.synchronize()
        return a.batch * a.batches / (time.perf_counter() - t0)

    run(False), run(True)   # warm-up: workspaces, staging buffers, graph records of both prompt forms
    rates = {False: [], True: []}
    for _ in range(a.rounds):
        for per_image in (False, True):
            rates[per_image].append(run(per_image))
    fixed, per = float(np.median(rates[False])), float(np.median(rates[True]))
    print(f"process_stream {a.size}x{a.size}, batch {a.batch}, {a.batches} batches, graph=True: fixed prompt {fixed:.2f} img/s, one prompt per image "
          f"{per:.2f} img/s ({100 * (per / fixed - 1):+.2f} %); rounds fixed {[round(r, 2) for r in rates[False]]} per-image {[round(r, 2) for r in rates[True]]}")


if __name__ == "__main__":
    main()
