#!/usr/bin/env python3
"""The two degradations on the device (ir_degrade: --degrade lq; ir_degrade_chain: --degrade realesrgan) measured:

  1. HIP-event time per image of both calls on 512 x 512 and 2048 x 2048 ground truth, with warm-up and `--repeats` timed event pairs, for
     `--draws` files' drawn parameters each (a chain's cost depends on what was drawn: the sizes of its intermediate images, Poisson or Gaussian
     noise); the 512 x 512 results are compared with the numpy model (tools/degrade_folder.py) before anything is timed.
  2. The same as a share of the network step that follows it: events around ir_pipeline alone at 2048 x 2048, the 512 -> 2048 product step,
     measured in the same process.
  3. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs):
     three runs with --degrade lq on --baseline_root (a built checkout of the parent commit; default this tree), then three runs with
     --degrade realesrgan on this tree. The allowance of the comparison is the baseline's own run-to-run spread (max - min of its three runs).

    python tools/bench_degrade.py [--files 16] [--repeats 10] [--draws 4] [--skip_cli] [--baseline_root DIR] [--out FILE]"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)
from tools import degrade_folder as M  # noqa: E402

EDGE = 2048


def _image(edge, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:edge, 0:edge].astype(np.float32)
    base = np.stack([127 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0), 127 + 80 * np.sin((xx + yy) / 71.0), 127 + 100 * np.cos(xx / 29.0 - yy / 41.0)], -1)
    return np.clip(np.rint(base + rng.normal(0, 3.0, base.shape)), 0, 255).astype(np.uint8)


def _timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def step_time(a, say):
    """The network step at 2048 x 2048, ir_pipeline alone with its input resident on the device."""
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
    ms = _timed(lambda: _launch_pipeline(ctx, st, 0, 1, EDGE, EDGE, flags, 512, 448, acp, sf, False), a.step_repeats)
    say(f"network step at {EDGE} x {EDGE} (ir_pipeline alone, input resident on the device): {spread(ms)}")
    return ctx, sds, statistics.median(ms)


def kernel_leg(a):
    import torch
    from instarevive_amd import degrade as D
    ctx, sds, step = step_time(a, say)
    recipes = {"lq": D.load_recipe("lq"), "realesrgan": D.load_recipe("realesrgan")}
    for edge in (512, 2048):
        img = _image(edge, edge)
        for kind, rec in recipes.items():
            meds = []
            for i in range(a.draws):
                p = D.draw(rec, f"bench_{i}.png", edge, edge, 231)
                chain = isinstance(p, D.ChainParams)
                host = np.zeros(((img.size + 255) & ~255) + D.extra_bytes(p), dtype=np.uint8)
                host[:img.size] = img.reshape(-1)
                k_at, n_at, _ = D.pack_extras(p, host, (img.size + 255) & ~255)
                dev = torch.from_numpy(host).to(ctx.device)
                out = torch.zeros(img.size, dtype=torch.uint8, device=ctx.device)
                if chain:
                    recs, sizes = [D.chain_record(p, dev.data_ptr(), k_at, D._device_tables(ctx).data_ptr())], D.check_chain(p, edge, edge)
                    fn = lambda: D.launch_chain(ctx, dev.data_ptr(), out.data_ptr(), edge, 3 * edge, edge, edge, recs, sizes)   # noqa: E731
                else:
                    recs = [D.record(p, dev.data_ptr() + k_at, dev.data_ptr() + n_at if n_at is not None else None)]
                    fn = lambda: D.launch(ctx, dev.data_ptr(), out.data_ptr(), edge, 3 * edge, edge, edge, recs)   # noqa: E731
                fn()
                torch.cuda.synchronize()
                if edge == 512 and i == 0:
                    got = out.cpu().numpy().reshape(edge, edge, 3)
                    want = M.degrade_chain_model(img, p.ops) if chain else M.degrade_model(img, p.kernel, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm)
                    assert np.array_equal(got, want), f"{kind}: the device image differs from the model's"
                ms = _timed(fn, a.repeats)
                meds.append(statistics.median(ms))
                what = p.describe() if chain else f"{p.kind} blur, to {p.lw} x {p.lh}, sigma {p.sigma:.1f}, q {p.q}"
                say(f"{'ir_degrade_chain' if chain else 'ir_degrade'} on {edge} x {edge}, file {i} ({what}): {spread(ms)}")
            med = statistics.median(meds)
            say(f"--degrade {kind} on {edge} x {edge} ground truth: median of {a.draws} files' medians {med:.3f} ms per image (least {min(meds):.3f}, most {max(meds):.3f})"
                + (f"; {100 * med / step:.2f} % of the {EDGE} x {EDGE} step's {step:.2f} ms" if edge == 512 else ""))
    return sds


def cli_leg(a, sds):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_degrade_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)   # 512 x 512 files, here the ground truth
        for how in ("lq", "lq", "lq", "realesrgan", "realesrgan", "realesrgan"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "lq" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu", "--degrade", how] + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"--degrade {how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            say(f"--degrade {how:<10} ({'this tree' if root == ROOT else 'the parent commit, built'}): {c['files_per_s']:.2f} files/s overall, "
                f"{c['steady_files_per_s']:.2f} after the first result, results left the GPU at {c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads)")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("lq") and rates.get("realesrgan"):
        base, mine = rates["lq"], rates["realesrgan"]
        spread_base = max(base) - min(base)
        say(f"--degrade realesrgan {[round(v, 3) for v in mine]} files/s, --degrade lq (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is "
            f"{spread_base:.3f} files/s ({100 * spread_base / statistics.median(base):.1f} %); median {statistics.median(mine):.3f} against "
            f"{statistics.median(base):.3f} ({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs with --degrade lq (default: this tree)")
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
