#!/usr/bin/env python3
"""MANIQA on the device (ir_maniqa, --maniqa_model) measured against the host model of the same tree (tools/evaluate_maniqa.py), with seeded
weights at the real shapes (ViT-B/8 with 10 blocks run, taps 6 .. 9, C = 3072, Swin stages at 768 and 384, 20 crops; the pretrained file does
not exist offline):

  1. The algorithmic cost, counted from the definition: multiply-accumulates of the trunk, the four TABs, the two Swin stages and the heads per
     crop, and the time an image's crops take at the fp32-MFMA peak. The cost does not depend on the image size.
  2. HIP-event time of ir_maniqa for one 2048 x 2048 result and for a batch of four 512 x 512 results, with warm-up, `--repeats` timed event
     pairs of BATCH calls over rotating inputs, the fraction of the fp32 floor reached, next to the network step (events around ir_pipeline
     alone) measured in the same process. The 2048 x 2048 result is compared with the fp32 CPU model before it is timed.
  3. The CPU fp32 model's time for one image.
  4. files/s of the command line (inference.py --sr_scale 4 --png_encoder gpu --resize gpu as a child process over K synthetic 512 x 512 PNGs):
     three runs without --maniqa_model, on --baseline_root (a built checkout of the parent commit; default this tree), then three runs with it
     on this tree. The allowance of the comparison is the baseline's own run-to-run spread (max - min of its three runs); both are printed.

    python tools/bench_maniqa.py [--files 16] [--repeats 5] [--skip_cli] [--skip_host] [--baseline_root DIR] [--out FILE]"""
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
from tools import evaluate_maniqa as EM  # noqa: E402

EDGE = 2048
BATCH = 2
SHAPES = [(2048, 1), (512, 4)]   # (edge, n)
PEAK_FP32_MFMA = 157.3e12        # FLOP/s of v_mfma_f32_32x32x2_f32 on an MI355X
CFG = dict(crop=224, patch=8, embed=768, vit_heads=12, vit_mlp=3072, vit_layers=10, taps=(6, 7, 8, 9), window=4, swin_heads=4, swin_depth=2, dim_mlp=768,
           scale=0.8, crops=20)


def seeded_model(seed=1357):
    import torch
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in EM.model_keys(CFG).items():
        if k in ("vit.pos_embed", "vit.cls_token") or k.endswith(".rpb"):
            sd[k] = torch.randn(shape, generator=g) * 0.5
        elif len(shape) >= 2:
            n_in = 1
            for v in shape[1:]:
                n_in *= v
            sd[k] = torch.randn(shape, generator=g) * n_in ** -0.5
        elif ".ln" in k and k.endswith(".weight"):
            sd[k] = torch.rand(shape, generator=g) + 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    for n, gain in (("score", 0.003), ("weight", 0.002)):   # the heads stay alive behind tokens that grow from stage to stage
        sd[n + ".fc2.weight"] = sd[n + ".fc2.weight"] * gain
    sd["score.fc2.bias"] = sd["score.fc2.bias"] * 0 + 1.0
    return EM.load_model(sd, {k: CFG[k] for k in ("taps", "scale", "crops", "vit_heads", "swin_heads")})


def macs():
    """(trunk, TABs, Swin stages and convs, heads) multiply-accumulates of ONE crop."""
    E, M, N = CFG["embed"], CFG["vit_mlp"], (CFG["crop"] // CFG["patch"]) ** 2
    T = N + 1
    trunk = N * 3 * CFG["patch"] ** 2 * E + CFG["vit_layers"] * (T * (4 * E * E + 2 * E * M) + 2 * T * T * E)
    tabs = sum(2 * (C * 3 * N * N + 2 * C * C * N) for C in (4 * E, E))
    swin = 0
    for cin, D, mlp in ((4 * E, E, CFG["dim_mlp"]), (E, E // 2, CFG["dim_mlp"] // 2)):
        swin += N * cin * D + EM.SWIN_LAYERS * CFG["swin_depth"] * (N * (4 * D * D + 2 * D * mlp) + 2 * N * CFG["window"] ** 2 * D)
    heads = N * 2 * ((E // 2) ** 2 + E // 2)
    return trunk, tabs, swin, heads


def kernel_leg(a):
    import torch
    import bench
    from instarevive_amd import _lib as L, maniqa
    from instarevive_amd.pipeline import _Staging, _launch_pipeline, _pipeline_flags, _prepare_fused
    parts = macs()
    per_image = 2 * sum(parts) * CFG["crops"]
    say(f"algorithmic cost of one crop: trunk {2 * parts[0] / 1e9:.1f} GFLOP + TABs {2 * parts[1] / 1e9:.1f} + Swin stages {2 * parts[2] / 1e9:.1f} + heads "
        f"{2 * parts[3] / 1e9:.2f} = {2 * sum(parts) / 1e9:.0f} GFLOP; an image of {CFG['crops']} crops {per_image / 1e12:.2f} TFLOP, whatever its size; "
        f"{1e3 * per_image / PEAK_FP32_MFMA:.1f} ms at the {PEAK_FP32_MFMA / 1e12:.1f} TF fp32-MFMA peak")
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
    maniqa.configure(ctx, model)
    for edge, n in SHAPES:
        img = _image(edge, edge)
        org = EM.crop_origins(edge, edge, CFG["crop"], CFG["crops"])
        want = None
        if edge == EDGE and not a.skip_host:
            t0 = time.perf_counter()
            want = EM.maniqa(img, model, org)
            t1 = time.perf_counter()
            say(f"CPU fp32 model (tools/evaluate_maniqa.py, torch, {torch.get_num_threads()} threads) on one image of {CFG['crops']} crops: {t1 - t0:.2f} s")
        per_pass = maniqa.crops_per_pass(ctx, n, CFG["crops"])
        need = maniqa.ws_bytes(ctx, n, CFG["crops"], per_pass)
        say(f"workspace of ir_maniqa for n = {n} ({per_pass} crops per pass; one crop per pass: {maniqa.ws_bytes(ctx, n, CFG['crops'], 1)} bytes): {need} bytes")
        rotate = 2
        t = torch.from_numpy(img).to(device)
        ins = [t.expand(n, -1, -1, -1).contiguous() for _ in range(rotate)]
        dorg = torch.tensor([org] * n, dtype=torch.int32, device=device)
        out = torch.zeros((n,), dtype=torch.float64, device=device)
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        nth = [0]

        def call():
            k = nth[0] % rotate
            nth[0] += 1
            ctx.check(ctx.lib.ir_maniqa(ctx.h, ctx.stream(), L.ptr(ins[k]), edge, 3 * edge, n, edge, edge, L.ptr(dorg), CFG["crops"], L.ptr(out), None, L.ptr(ws),
                                        ws.numel()), "ir_maniqa")
        call()
        torch.cuda.synchronize()
        got = out.cpu().tolist()
        assert all(v == got[0] for v in got), got
        dev = abs(got[0] - want) if want is not None else float("nan")
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
        floor = 1e3 * n * per_image / PEAK_FP32_MFMA
        say(f"ir_maniqa {edge} x {edge}, n = {n} ({rotate} rotating inputs, per call of {BATCH} per event pair; score {got[0]:.9f}, "
            f"{'%.1e from the CPU fp32 model' % dev if want is not None else 'not compared'}): {spread(ms)}; {100 * floor / med:.1f} % of the fp32 floor "
            f"({floor:.1f} ms); per image {100 * med / n / step:.1f} % of the {EDGE} x {EDGE} step's {step:.2f} ms")
        del ins, ws
    return sds, model


def cli_leg(a, sds, model):
    from tools import cli_artifacts as A
    d = tempfile.mkdtemp(prefix="ir_maniqa_cli_")
    rates = {}
    try:
        flags = A.write_full_artifacts(d, sds)
        A.write_lq_pngs(os.path.join(d, "in"), a.files)
        EM.save_npz(os.path.join(d, "maniqa.npz"), model)
        for how in ("base", "base", "base", "maniqa", "maniqa", "maniqa"):
            out = os.path.join(d, "out")
            shutil.rmtree(out, ignore_errors=True)
            root = (a.baseline_root or ROOT) if how == "base" else ROOT
            cmd = [sys.executable, os.path.join(root, "inference.py"), "--input", os.path.join(d, "in"), "--output", out, "--sr_scale", "4", "--png_encoder", "gpu",
                   "--resize", "gpu"] + (["--maniqa_model", os.path.join(d, "maniqa.npz")] if how == "maniqa" else []) + flags
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
            rate = A.parse_cli_rate(r.stdout)
            written = len([f for f in os.listdir(out) if f.endswith(".png")]) if os.path.isdir(out) else 0
            if r.returncode or not rate or written != a.files:
                say(f"{how}: FAILED (rc {r.returncode}, {written} of {a.files} files) {r.stderr[-400:]}")
                continue
            c = rate[0]
            avg = " ".join(ln for ln in r.stdout.splitlines() if ln.startswith("maniqa: "))
            say(f"{'with --maniqa_model   ' if how == 'maniqa' else 'without --maniqa_model'} ({'this tree' if root == ROOT else 'the parent commit, built'}): "
                f"{c['files_per_s']:.2f} files/s overall, {c['steady_files_per_s']:.2f} after the first result, results left the GPU at "
                f"{c.get('result_rate', float('nan')):.2f} /s ({c['workers']} host threads) {avg}")
            rates.setdefault(how, []).append(c["files_per_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    if rates.get("base") and rates.get("maniqa"):
        base, mine = rates["base"], rates["maniqa"]
        spread_base = max(base) - min(base)
        say(f"--maniqa_model {[round(v, 3) for v in mine]} files/s, without (baseline) {[round(v, 3) for v in base]}; the baseline's own spread is {spread_base:.3f} "
            f"files/s ({100 * spread_base / statistics.median(base):.1f} %); median with the flag {statistics.median(mine):.3f} against "
            f"{statistics.median(base):.3f} ({100 * (statistics.median(mine) / statistics.median(base) - 1):+.1f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step_repeats", type=int, default=5)
    ap.add_argument("--skip_cli", action="store_true")
    ap.add_argument("--skip_host", action="store_true", help="do not time the CPU model")
    ap.add_argument("--baseline_root", default=None, help="a built checkout of the parent commit for the runs without --maniqa_model (default: this tree)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    a.baseline_root = os.path.abspath(a.baseline_root) if a.baseline_root else None
    try:
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
