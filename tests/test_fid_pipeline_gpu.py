"""FID through the product: process(..., gt=, fid=True) on the reduced models, inference.py and eval_batch.py with --fid_model, and
tools/evaluate_fid.py --backend gpu over the folder a run wrote.

The gate of the distance, propagated from the feature gate g (tests/support/fid_model.py: max_c |f - ref| <= g max_c |ref| per image): the
square root d of the Frechet distance is the 2-Wasserstein distance of the two fitted Gaussians, a metric, so moving both feature sets moves d
by at most eta_1 + eta_2, eta = the distance between a set's Gaussian and its moved Gaussian. Pairing every feature with its moved twin is a
coupling whose cost bounds that distance: eta^2 <= N / (N - 1) max_i |f_i - ref_i|^2 <= N / (N - 1) 2048 (g F)^2 with F the largest |ref| (the
factor N / (N - 1) is the covariance's ddof 1). With the reference's statistics fixed (--fid_stats) only one side moves. Hence
|d'^2 - d^2| <= 2 k eta d + (k eta)^2 with k = 2 (two sets) or 1, plus half a unit of the printed fifth decimal. Recorded in docs/parity.md."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests.support import fid_model as FM

pytestmark = pytest.mark.gpu
EF = FM.EF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 64), (40, 56), (64, 64), (33, 90), (72, 72), (50, 50)]
_made = {}


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _distance_gate(ref_sets, value, sides):
    g, n = FM.feature_gate(), min(len(s) for s in ref_sets)
    eta = np.sqrt(n / (n - 1.0) * 2048) * g * max(np.abs(s).max() for s in ref_sets)
    return 2 * sides * eta * np.sqrt(max(value, 0.0)) + (sides * eta) ** 2 + 0.5e-5


def _folder(tmp_path_factory):
    """Once per module: the model artefacts, six inputs of five sizes with a mirrored ground-truth tree, the Inception weights as an .npz."""
    if "d" not in _made:
        from tests.golden._det import det_input
        from tests.support.metrics_model import ramp
        from tests.test_cli_gpu import _write_artifacts
        d = tmp_path_factory.mktemp("fid_cli")
        _write_artifacts(d)
        truth = {}
        for i, hw in enumerate(SIZES):
            sub = ("", "deep/")[i % 2]
            os.makedirs(d / "in" / sub, exist_ok=True)
            os.makedirs(d / "gt" / sub, exist_ok=True)
            Image.fromarray((det_input(500 + i, hw + (3,)) * 255).numpy().astype(np.uint8)).save(d / "in" / f"{sub}im{i:02d}.png")
            truth[f"{sub}im{i:02d}_0.png"] = ramp(hw[0], hw[1], 700 + i)
            Image.fromarray(truth[f"{sub}im{i:02d}_0.png"]).save(d / "gt" / f"{sub}im{i:02d}.png")
        np.savez(d / "inception.npz", **{k: v.numpy() for k, v in FM.weights().items()})
        cmd = [sys.executable, os.path.join(ROOT, "inference.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "in"), "--swinir_ckpt",
               str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
               "--prompt_embeds", str(d / "prompt.pth"), "--batch_size", "3", "--workers", "4", "--png_encoder", "gpu", "--resize", "gpu"]
        _made.update(d=d, truth=truth, cmd=cmd)
    return _made["d"], _made["truth"], _made["cmd"]


def _host_features(images):
    return FM.model("fp64").features_of_images(images, "clean", 6)


def _saved(folder, keys):
    return [np.array(Image.open(folder / k).convert("RGB")) for k in keys]


def test_process_returns_the_features_of_its_images_and_of_the_ground_truth():
    """process(..., gt=, fid=True) on the reduced models: the last element holds ir_fid_features of the returned predictions and of the ground
    truth, to the bit; without fid the result is what it was."""
    from instarevive_amd import fid as G
    from instarevive_amd.pipeline import process
    from tests import test_models_gpu as T
    from tests.golden._det import det_input
    from tests.support.metrics_model import ramp
    (sw, _), (vae, _), (dit, _) = T._small_models()
    y, mask3 = T._prompt(T.DIT_SMALL)
    imgs = [(det_input(60 + i, (64, 128, 3)) * 255).numpy().astype(np.uint8) for i in range(2)]
    gts = [ramp(64, 128, 40 + i) for i in range(2)]
    kw = dict(preprocess_model=sw, vae=vae, y=y.cuda(), y_mask=mask3.cuda())
    with pytest.raises(ValueError, match="no Inception weights"):
        dit.ctx.__dict__.pop("_fid_ready", None)
        process(dit, imgs, 1, "wavelet", False, False, 512, 448, gt=gts, fid=True, **kw)
    G.configure(dit.ctx, FM.weights())
    out = process(dit, imgs, 1, "wavelet", False, False, 512, 448, gt=gts, fid=True, **kw)
    plain = process(dit, imgs, 1, "wavelet", False, False, 512, 448, gt=gts, **kw)
    assert len(out) == 4 and len(plain) == 3 and out[2] == plain[2] and all(np.array_equal(a, b) for a, b in zip(out[0], plain[0]))
    extra = out[3]
    assert sorted(extra) == ["fid", "fid_gt"] and extra["fid"].shape == extra["fid_gt"].shape == (2, 2048)
    for i in range(2):
        assert np.array_equal(_bits(extra["fid"][i]), _bits(G.fid_arrays(dit.ctx, out[0][i])[0]))
        assert np.array_equal(_bits(extra["fid_gt"][i]), _bits(G.fid_arrays(dit.ctx, gts[i])[0]))
    alone = process(dit, imgs, 1, "wavelet", False, False, 512, 448, fid="legacy", **kw)
    assert len(alone) == 3 and alone[2]["fid_gt"] is None
    assert np.array_equal(_bits(alone[2]["fid"][1]), _bits(G.fid_arrays(dit.ctx, alone[0][1], "legacy")[0]))


def test_inference_prints_the_fid_of_the_saved_files_and_leaves_the_csv_alone(tmp_path_factory):
    """inference.py --gt --fid_model over six files: the last averages line is `fid:` and equals frechet_distance of the float64 model's features
    of the decoded saved PNGs and of the ground truth within the propagated gate; the feature file holds the device's features of those files
    within the feature gate; metrics.csv is byte-identical to a run without the flag."""
    from tests.test_metrics_gpu import _run
    d, truth, cmd = _folder(tmp_path_factory)
    stdout = _run(cmd + ["--gt", str(d / "gt"), "--output", str(d / "out"), "--fid_model", str(d / "inception.npz")])
    plain = _run(cmd + ["--gt", str(d / "gt"), "--output", str(d / "plain")])
    assert (d / "out" / "metrics.csv").read_bytes() == (d / "plain" / "metrics.csv").read_bytes()
    assert "fid: " not in plain and "--fid_model" not in plain and not (d / "plain" / "fid_features.npz").exists()
    assert "--fid_model: 6 files entered the set, 0 did not" in stdout, stdout[-1500:]
    avg = [ln for ln in stdout.splitlines() if ln.startswith(("psnr: ", "ssim: ", "fid: "))]
    assert [ln.split(":")[0] for ln in avg] == ["psnr", "ssim", "fid"]
    assert any("rank-deficient" in ln and "equal N" in ln for ln in stdout.splitlines())
    keys = sorted(truth)
    ref_p, ref_g = _host_features(_saved(d / "out", keys)), _host_features([truth[k] for k in keys])
    want = EF.frechet_distance(*EF.statistics(ref_p), *EF.statistics(ref_g))
    got, gate = float(avg[2].split()[1]), _distance_gate([ref_p, ref_g], want, 2)
    print(f"fid of the run {got:.5f}, of the float64 model over the saved files {want:.9f}, off by {abs(got - want):.2e} (propagated gate {gate:.2e})")
    assert abs(got - want) <= gate
    assert (d / "out" / "fid.txt").read_text() == avg[2] + "\n"
    with np.load(d / "out" / "fid_features.npz") as z:
        order = [str(s) for s in z["names"]]   # a rank's file keeps the order its files were processed in; merge() sorts by name
        assert sorted(order) == keys and order == [str(s) for s in z["gt_names"]]
        for dev, ref in ((z["features"], ref_p), (z["gt_features"], ref_g)):
            assert all(FM.measure(dev[order.index(k)], ref[i]) <= FM.feature_gate() for i, k in enumerate(keys))
        assert f"fid: {EF.frechet_distance(*EF.statistics(z['features']), *EF.statistics(z['gt_features'])):.5f}" == avg[2]


def test_fid_stats_needs_no_ground_truth_and_the_tool_agrees(tmp_path_factory):
    """--fid_stats without --gt: no metrics.csv, the `fid:` line against the saved statistics within the propagated gate (one side moves);
    tools/evaluate_fid.py --backend gpu over the output folder prints the same line."""
    from tests.test_metrics_gpu import _run
    d, truth, cmd = _folder(tmp_path_factory)
    rng = np.random.default_rng(3)
    base = FM.reference("64x48")[0]
    mu, sigma = EF.statistics(base[None] * (1 + 0.2 * rng.normal(0, 1, (12, 2048))))
    np.savez(d / "stats.npz", mu=mu, sigma=sigma)
    stdout = _run(cmd + ["--output", str(d / "st"), "--fid_model", str(d / "inception.npz"), "--fid_stats", str(d / "stats.npz")])
    assert not (d / "st" / "metrics.csv").exists() and "--fid_model: 6 files entered the set, 0 did not" in stdout, stdout[-1500:]
    line = [ln for ln in stdout.splitlines() if ln.startswith("fid: ")]
    assert len(line) == 1
    keys = sorted(truth)
    ref_p = _host_features(_saved(d / "st", keys))
    want = EF.frechet_distance(*EF.statistics(ref_p), mu, sigma)
    got, gate = float(line[0].split()[1]), _distance_gate([ref_p], want, 1)
    print(f"fid against the statistics {got:.5f}, float64 model {want:.9f}, off by {abs(got - want):.2e} (propagated gate {gate:.2e})")
    assert abs(got - want) <= gate
    tool = _run([sys.executable, os.path.join(ROOT, "tools", "evaluate_fid.py"), "--model", str(d / "inception.npz"), str(d / "st"), "--stats", str(d / "stats.npz"),
                 "--backend", "gpu"])
    assert tool.splitlines()[-1] == line[0], tool[-500:]
    assert _run([sys.executable, os.path.join(ROOT, "tools", "evaluate_fid.py"), "--features", str(d / "st" / "fid_features.npz"), "--stats",
                 str(d / "stats.npz")]).splitlines()[-1] == line[0]


def test_eval_batch_takes_the_flag(tmp_path_factory):
    """eval_batch.py --gt --fid_model: one `fid:` line, behind both reports' averages, of the restored folder against the cropped ground truth."""
    from instarevive_amd.utils import center_crop_arr
    from tests.test_metrics_gpu import _run
    d, truth, _ = _folder(tmp_path_factory)
    names = sorted(os.listdir(d / "gt"))   # the top-level files: im00, im02, im04
    os.makedirs(d / "lq2", exist_ok=True)
    os.makedirs(d / "gt2", exist_ok=True)
    for k in names:
        if k.endswith(".png"):
            Image.open(d / "in" / k).save(d / "lq2" / k)
            g = np.array(Image.open(d / "gt" / k).convert("RGB"))
            Image.fromarray(np.pad(g, ((0, 9), (0, 5), (0, 0)), mode="edge")).save(d / "gt2" / k)
    files = sorted(k for k in names if k.endswith(".png"))
    stdout = _run([sys.executable, os.path.join(ROOT, "eval_batch.py"), "--ckpt", str(d / "weights" / "dit.ckpt"), "--input", str(d / "lq2"), "--output",
                   str(d / "res"), "--cond_output", str(d / "cond"), "--batch_size", "2", "--image_size", "64", "--swinir_ckpt",
                   str(d / "weights" / "swinir.ckpt"), "--swinir_config", str(d / "swinir.yaml"), "--vae", str(d / "vae"), "--dit_config", str(d / "pixart"),
                   "--prompt_embeds", str(d / "prompt.pth"), "--gt", str(d / "gt2"), "--fid_model", str(d / "inception.npz")])
    lines = stdout.splitlines()
    fid_lines = [i for i, ln in enumerate(lines) if ln.startswith("fid: ")]
    assert len(fid_lines) == 1 and fid_lines[0] > max(i for i, ln in enumerate(lines) if ln.startswith("ssim: ")), stdout[-1500:]
    assert f"--fid_model: {len(files)} files entered the set, 0 did not" in stdout
    assert (d / "res" / "metrics.csv").read_text().splitlines()[0] == "file,psnr_y,ssim_y"
    crops = [np.ascontiguousarray(center_crop_arr(Image.open(d / "gt2" / k).convert("RGB"), 64)) for k in files]
    ref_p, ref_g = _host_features(_saved(d / "res", files)), _host_features(crops)
    want = EF.frechet_distance(*EF.statistics(ref_p), *EF.statistics(ref_g))
    got = float(lines[fid_lines[0]].split()[1])
    print(f"eval_batch fid {got:.5f}, float64 model {want:.9f}")
    assert abs(got - want) <= _distance_gate([ref_p, ref_g], want, 2)
