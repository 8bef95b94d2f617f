#!/usr/bin/env python3
"""TOPIQ-NR on the device (ir_topiq, --topiq_model) measured against the host model of the same tree (tools/evaluate_topiq.py), with seeded
weights at the real widths (width 64, depths 3 / 4 / 6 / 3, D = 256, 4 heads, FFN 2048; the pretrained file does not exist offline):

  1. The algorithmic cost, DERIVED from the bound shapes: multiply-accumulates of the trunk, the five gates, the reductions and the ten
     attention layers, and the time they take at the fp32-MFMA peak. It is printed next to every measured time.
  2. HIP-event time of ir_topiq for one 2048 x 2048 result and for a batch of four 512 x 512 results, with warm-up, `--repeats` timed event
     pairs of BATCH calls over rotating inputs, the fraction of the fp32 floor reached, next to the network step (events around ir_pipeline
     alone) measured in the same process. Every result is compared with the fp32 CPU model before it is timed.
  3. The CPU fp32 model's time for the same images.
  4. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs):
     three runs without --topiq_model, on --baseline_root (a built checkout of the parent commit; default this tree), then three runs with it
     on this tree. The allowance of the comparison is the baseline's own run-to-run spread (max - min of its three runs); both are printed.

    python tools/bench_topiq.py [--files 16] [--repeats 10] [--skip_cli] [--skip_host_2048] [--baseline_root DIR] [--out profiles/topiq.txt]"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_png import LINES, say, spread  # noqa: E402  (one report format for the side-work tools)
from tools.bench_clipiqa import _image  # noqa: E402
from tools import evaluate_topiq as ET  # noqa: E402

EDGE = 2048
BATCH = 4
SHAPES = [(2048, 1), (512, 4)]   # (edge, n)
PEAK_FP32_MFMA = 157.3e12        # FLOP/s of v_mfma_f32_32x32x2_f32 on an MI355X
CFG = dict(width=64, depths=(3, 4, 6, 3), dim=256, heads=4, ffn=2048)


def seeded_model(seed=8765, cfg=CFG):
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in ET.model_keys(cfg).items():
        if k in ("h_emb", "w_emb"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) >= 2:
            fan = 1
            for v in shape[1:]:
                fan *= v
            sd[k] = torch.randn(shape, generator=g) * (2.0 ** 0.5 if k.startswith("trunk.") else 1.0) * fan ** -0.5
        elif k.endswith("running_var") or (k.endswith(".weight") and (".bn" in k or "downsample.1" in k or ".norm" in k or k in ("score.0.weight", "score.3.weight"))):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    return ET.load_model(sd, cfg["heads"])


def macs(h, w, cfg=CFG):
    """(trunk, gates, reductions, attention layers) multiply-accumulates of one h x w image, from the model's shapes alone."""
    W, D, Fn = cfg["width"], cfg["dim"], cfg["ffn"]
    sizes, tokens = ET.level_sizes(h, w), ET.token_sizes(h, w)
    trunk = sizes[0][0] * sizes[0][1] * 147 * W
    H, Wd = ET.down2(sizes[0][0]), ET.down2(sizes[0][1])
    inplanes = W
    for l, depth in enumerate(cfg["depths"]):
        planes = W << l
        for b in range(depth):
            s = ET.STRIDES[l] if b == 0 else 1
            Ho, Wo = (ET.down2(H), ET.down2(Wd)) if s == 2 else (H, Wd)
            trunk += H * Wd * inplanes * planes + Ho * Wo * (9 * planes * planes + planes * 4 * planes) + (Ho * Wo * inplanes * 4 * planes if b == 0 else 0)
            inplanes, H, Wd = 4 * planes, Ho, Wo
    gates = reduce = 0
    for (Hi, Wi), (th, tw), C in zip(sizes, tokens, ET.level_channels(W)):
        gates += Hi * Wi * (C * 2 * C + C * ET.GATE_HIDDEN + 9 * ET.GATE_HIDDEN * ET.GATE_HIDDEN + 9 * ET.GATE_HIDDEN)
        reduce += th * tw * C * D
    T = [a * b for a, b in tokens]

    def enc(t):
        return t * (4 * D * D + 2 * D * Fn) + 2 * t * t * D

    attn = sum(enc(t) for t in T) + enc(T[4])
    for k in range(4):
        attn += T[4] * (2 * D * D + 2 * D * Fn) + T[3 - k] * 2 * D * D + 2 * T[4] * T[3 - k] * D
    return trunk, gates, reduce, attn


def cost_line(edge):
    t, g, r, a = macs(edge, edge)
    total = t + g + r + a
    return (f"derived cost of one {edge} x {edge} image ({ET.token_sizes(edge, edge)[4][0] * ET.token_sizes(edge, edge)[4][1]} tokens per level): trunk {t / 1e9:.1f} GMAC + "
            f"gates {g / 1e9:.1f} + reductions {r / 1e9:.2f} + attention layers {a / 1e9:.1f} = {total / 1e9:.0f} GMAC = {2 * total / 1e12:.2f} TFLOP; "
            f"{1e3 * 2 * total / PEAK_FP32_MFMA:.2f} ms at the {PEAK_FP32_MFMA / 1e12:.1f} TF fp32-MFMA peak")


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L, topiq
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    for edge, n in SHAPES:
        say(cost_line(edge))
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
    model = seeded_model()
    topiq.configure(ctx, model)
    for edge, n in SHAPES:
        img = _image(edge, edge)
        want = None
        if edge < 2048 or not a.skip_host_2048:
            t0 = time.perf_counter()
            want = ET.topiq(img, model)
            t1 = time.perf_counter()
            say(f"CPU fp32 model (tools/evaluate_topiq.py, torch, {torch.get_num_threads()} threads) on one {edge} x {edge} image: {t1 - t0:.3f} s"
                + (f"; a batch of {n}: {n * (t1 - t0):.3f} s" if n > 1 else ""))
        else:
            say(f"CPU fp32 model on one {edge} x {edge} image: not measured (--skip_host_2048)")
        need = topiq.ws_bytes(ctx, n, edge, edge)
        say(f"workspace of ir_topiq for n = {n} of {edge} x {edge}: {need} bytes")
        rotate = 2
        t = torch.from_numpy(img).to(device)
        ins = [t.expand(n, -1, -1, -1).contiguous() for _ in range(rotate)]
        out = torch.zeros((n,), dtype=torch.float64, device=device)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_topiq(ctx.h, ctx.stream(), L.ptr(ins[k]), edge, 3 * edge, n, edge, edge, L.ptr(out), None, None, L.ptr(ws), ws.numel()), "ir_topiq")
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        got = out.cpu().tolist()
        assert all(v == got[0] for v in got), got
        dev = abs(got[0] - want) if want is not None else float("nan")
        assert want is None or dev < 1e-4, (got[0], want)
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
        floor = 1e3 * n * 2 * sum(macs(edge, edge)) / PEAK_FP32_MFMA
        say(f"ir_topiq {edge} x {edge}, n = {n} ({rotate} rotating inputs, per call of {BATCH} per event pair; score {got[0]:.9f}, "
            f"{'%.1e from the CPU fp32 model' % dev if want is not None else 'not compared'}): {spread(ms)}; derived floor {floor:.2f} ms, measured {med:.2f} ms = "
            f"{100 * floor / med:.1f} % of the fp32 floor; per image {100 * med / n / step:.1f} % of the {EDGE} x {EDGE} step's {step:.2f} ms")
        del ins, ws
    return sds, model


def cli_leg(a, sds, model):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_topiq_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        ET.save_npz(os.path.join(d, "topiq.npz"), model)
        for how in ("base", "base", "base", "topiq", "topiq", "topiq"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu"] + (["--topiq_model", os.path.join(d, "topiq.npz")] if how == "topiq" else []) + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith("topiq_nr: "))
            say(f"{'with --topiq_model   ' if how == 'topiq' else 'without --topiq_model'} ({'this tree' if root == ROOT else 'the parent commit, built'}): "
                f"{c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("topiq"):
        base, mine = rates["base"], rates["topiq"]
        spread_base = max(base) - min(base)
        say(f"--topiq_model {[round(v, 3) for v in mine]} files/s, without (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is {spread_base:.3f} "
            f"files/s ({100 * spread_base / statistics.median(base):.1f} %); median with the flag {statistics.median(mine):.3f} against "
            f"{statistics.median(base):.3f} ({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--skip_host_2048", action="store_true", help="do not time the CPU model at 2048 x 2048")
    ap.add_argument("--cost_only", action="store_true", help="print the derived cost and stop (needs no GPU)")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --topiq_model (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    try:
        if a.cost_only:
            for edge, _ in SHAPES:
                say(cost_line(edge))
            return
        sds, model = kernel_leg(a)
        if not a.skip_cli:
            cli_leg(a, sds, model)
    finally:
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
