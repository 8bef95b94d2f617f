#!/usr/bin/env python3
"""Time ir_fid_features on one MI355X and write profiles/fid.txt.

  1. the call: HIP events around ir_fid_features for one 2048 x 2048 result and for a batch of four 512 x 512 results, medians over
     `--repeats` timed calls over rotating inputs behind `--warmup` calls, as a fraction of the fp32-MFMA floor. The algorithmic cost is
     derived, not measured: evaluate_fid.macs_per_image() = 5 711 168 096 MAC per image over the 94 convolutions whatever the image's size
     (the network always sees 299 x 299), 11.42 GFLOP, 0.0726 ms at 157.3 TF;
  2. the share of the network step: against the 2048 x 2048 step recorded in profiles/dists.txt (115.91 ms; this tool does not load the
     restoration models);
  3. the CPU fp32 model (tools/evaluate_fid.py::InceptionFID, resize included) for the same image, and the deviation between the two.

The weights are seeded at Inception-v3's real widths (tests/support/fid_model.py); timing does not depend on their values. The files/s of the
command line with --fid_model against the built parent commit are not measured by this tool yet.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_FLOPS = 157.3e12
STEP_MS = 115.91   # profiles/dists.txt: the 2048 x 2048 network step


def _image(edge, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge]
    base = np.stack([127 + 90 * np.sin(xx / (13.0 + c) + seed) * np.cos(yy / (17.0 - c)) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid.txt"))
    a = ap.parse_args()
    import evaluate_fid as EF
    from instarevive_amd import fid as G
    from instarevive_amd.models import get_context
    from tests.support import fid_model as FM
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    device = torch.device("cuda", 0)
    ctx = get_context(device)
    G.configure(ctx, FM.weights())
    flop = 2.0 * EF.macs_per_image()
    say(f"derived: {EF.macs_per_image()} MAC per image = {flop / 1e9:.2f} GFLOP, {1e3 * flop / PEAK_FLOPS:.4f} ms at 157.3 TF (fp32 MFMA)")
    host_net = EF.InceptionFID(FM.weights(), "fp32")
    for edge, n in ((2048, 1), (512, 4)):
        rotate = 3
        imgs = [np.stack([_image(edge, 10 * k + j) for j in range(n)]) for k in range(rotate)]
        ins = [torch.from_numpy(x).to(device) for x in imgs]
        out = torch.zeros((n, G.DIM), dtype=torch.float64, device=device)
        ws = G.workspace(ctx, G.ws_bytes(n))
        ms = []
        for it in range(a.warmup + a.repeats):
            x = ins[it % rotate]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            G.queue_fid(ctx, x.data_ptr(), edge, 3 * edge, n, edge, edge, "clean", out, ws)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        med, floor = statistics.median(ms), 1e3 * n * flop / PEAK_FLOPS
        say(f"ir_fid_features {edge} x {edge}, {n} image(s) per call ({rotate} rotating inputs, workspace {G.ws_bytes(n) / 1e6:.1f} MB): median {med:.3f} ms "
            f"(min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} calls); {n * flop / med / 1e9:.2f} TF, {100 * floor / med:.2f} % of the {floor:.4f} ms floor; "
            f"per image {100 * med / n / STEP_MS:.2f} % of the recorded 2048 x 2048 step ({STEP_MS} ms)")
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        ref = host_net.features_of_images([imgs[(a.warmup + a.repeats - 1) % rotate][0]])
        dt = time.perf_counter() - t0
        say(f"  CPU fp32 model, one {edge} x {edge} image on {torch.get_num_threads()} threads: {dt:.3f} s; device against it: "
            f"{np.abs(got[0] - ref[0]).max() / np.abs(ref[0]).max():.2e} (max_c |d| / max_c |ref|)")
    say("command line: files/s with --fid_model against the built parent commit are not measured by this tool yet")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
