"""Generate tests/golden/degrade_chain.npz and tests/golden/realesrgan_val.json by RUNNING THE REFERENCE's own code (imported read-only):

    python tests/golden/make_degrade_chain_golden.py --reference REFERENCE_ROOT

Nothing from the reference is copied: the fixtures hold arrays and settings only.
  - the outputs of utils/degradation.py's kernel builders (bivariate_Gaussian, bivariate_generalized_Gaussian and bivariate_plateau, isotropic
    and not) and of circular_lowpass_kernel for fixed arguments;
  - utils/image/common.py:filter2D on a 24 x 31 image;
  - utils/image/diffjpeg.py on a 37 x 53 and a 16 x 16 image at the float32 qualities 30.5, 49.9 and 95: CompressJpeg(rounding=identity), i.e.
    the quotients before the rounding; DeCompressJpeg on the integer coefficients of THIS project's model (tools/degrade_folder.py), so that a
    near-tie cannot make the two sides decompress different integers; and DiffJPEG(differentiable=False) as a whole, with the mask of the
    8 x 8 blocks (16 x 16 where a chroma coefficient is the cause) that hold a coefficient whose fp64 quotient lies within 1e-4 of a tie -
    asserted here to be under 5 % of the blocks;
  - the parameters of configs/general_deg_realesrgan_val.yaml (the dataset's kernel settings and the batch transform's parameters, without the
    file list, crop, flips and training queue) as realesrgan_val.json.
cv2 and torchvision, which the modules import and these functions never call, are stubbed as make_degrade_golden.py does.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KERNEL_CASES = [("gauss", 13, 2.0, 0.7, 0.4, 0.0, False), ("generalized", 13, 1.7, 1.7, 0.0, 0.6, True), ("generalized", 21, 2.5, 0.9, -1.1, 2.7, False),
                ("plateau", 13, 1.2, 1.2, 0.0, 1.8, True), ("plateau", 9, 2.9, 0.5, 2.2, 1.1, False)]   # (family, K, sig_x, sig_y, theta, beta, isotropic)
SINC_CASES = [(1.3, 13, 21), (2.9, 7, 21), (0.7, 21, 0)]   # (cutoff, K, pad_to)
QUALITIES = [30.5, 49.9, 95.0]
JPEG_SHAPES = [(37, 53), (16, 16)]
TIE = 1e-4


def import_reference(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)

    def missing(attr):   # names the modules import and these functions never use
        if attr.startswith("__"):
            raise AttributeError(attr)
        return object

    def mk(name):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__["__getattr__"] = missing
        sys.modules[name] = m
    for name in ("cv2", "torchvision", "torchvision.transforms", "torchvision.transforms.functional_tensor"):
        mk(name)
    from utils import degradation
    from utils.image import diffjpeg
    from utils.image.common import filter2D
    return degradation, diffjpeg, filter2D


def test_image(rng, h, w):
    """A smooth image with texture, as bytes: blocks with few and with many non-zero coefficients."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.4 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], axis=-1)
    return np.clip(np.rint((base + rng.normal(0, 0.06, (h, w, 3))) * 255), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (read only)")
    ap.add_argument("--out", default=os.path.join(HERE, "degrade_chain.npz"))
    ap.add_argument("--recipe_out", default=os.path.join(HERE, "realesrgan_val.json"))
    a = ap.parse_args()
    ref = os.path.abspath(a.reference)
    D, J, filter2D = import_reference(ref)
    import torch
    import yaml
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import degrade_folder as M

    out = {}
    for i, (fam, K, sx, sy, th, beta, iso) in enumerate(KERNEL_CASES):
        fn = {"gauss": lambda: D.bivariate_Gaussian(K, sx, sy, th, isotropic=iso),
              "generalized": lambda: D.bivariate_generalized_Gaussian(K, sx, sy, th, beta, isotropic=iso),
              "plateau": lambda: D.bivariate_plateau(K, sx, sy, th, beta, isotropic=iso)}[fam]
        out[f"kernel_{i}"] = fn()
        assert out[f"kernel_{i}"].dtype == np.float64
    for i, (cutoff, K, pad) in enumerate(SINC_CASES):
        out[f"sinc_{i}"] = D.circular_lowpass_kernel(cutoff, K, pad_to=pad)

    rng = np.random.default_rng(20)
    img = test_image(rng, 24, 31)
    k = out["kernel_2"]
    x = M.to_float(img)
    with torch.no_grad():
        y = filter2D(torch.from_numpy(x).permute(2, 0, 1)[None].contiguous(), torch.from_numpy(k).float()[None])
    out["filter_img"], out["filter_out"] = img, y[0].permute(1, 2, 0).numpy()

    basis = M.dct_basis()
    for s, (h, w) in enumerate(JPEG_SHAPES):
        img = test_image(rng, h, w)
        out[f"jpeg_img_{s}"] = img
        x = M.to_float(img)
        H, W = (h + 15) & ~15, (w + 15) & ~15
        xt = torch.from_numpy(x).permute(2, 0, 1)[None].contiguous()
        xp = torch.nn.functional.pad(xt, (0, W - w, 0, H - h))
        for qi, q in enumerate(QUALITIES):
            f = M.jpeg_factor(q)
            ft = torch.tensor([float(f)], dtype=torch.float32)
            with torch.no_grad():
                quot = J.CompressJpeg(rounding=lambda v: v)(xp, factor=ft)
                planes = M.jpeg_planes(x)
                mine = [M.jpeg_quotients(p, M.JPEG_TABLES[min(c, 1)], f, basis) for c, p in enumerate(planes)]
                coef = [torch.from_numpy(np.rint(m).reshape(1, -1, 8, 8)) for m in mine]
                dec = J.DeCompressJpeg()(coef[0], coef[1], coef[2], H, W, factor=ft)
                full = J.DiffJPEG(differentiable=False)(xt, torch.tensor([q], dtype=torch.float32))
            # blocks with a near-tie, judged on the fp64 restatement's own quotients
            tie = [np.abs(m.astype(np.float64) - np.floor(m.astype(np.float64)) - 0.5).min(axis=1) < TIE for m in mine]
            mask = tie[0].reshape(H // 8, W // 8).copy()
            cm = (tie[1] | tie[2]).reshape(H // 16, W // 16)
            mask |= np.repeat(np.repeat(cm, 2, axis=0), 2, axis=1)
            assert mask.mean() < 0.05, f"{mask.mean():.3f} of the blocks of {h} x {w} at {q} hold a near-tie"
            for c, name in enumerate(("y", "cb", "cr")):
                out[f"jpeg_quot_{s}_{qi}_{name}"] = quot[c][0].numpy().reshape(-1, 64)
            out[f"jpeg_dec_{s}_{qi}"] = dec[0].permute(1, 2, 0).numpy()[:h, :w]
            out[f"jpeg_full_{s}_{qi}"] = full[0].permute(1, 2, 0).numpy()
            out[f"jpeg_tie_{s}_{qi}"] = mask
            print(f"{h} x {w} q {q}: {mask.mean() * 100:.1f} % of the blocks excluded")
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    assert size < 256 * 1024, size
    print(f"wrote {a.out} ({size} bytes)")

    with open(os.path.join(ref, "configs", "general_deg_realesrgan_val.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    rec = {"chain": "realesrgan"}
    rec.update({k: v for k, v in cfg["dataset"]["params"].items() if k not in ("file_list", "out_size", "crop_type", "use_hflip", "use_rot")})
    rec.update({k: v for k, v in cfg["batch_transform"]["params"].items() if k != "queue_size"})
    with open(a.recipe_out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {a.recipe_out}")


if __name__ == "__main__":
    main()
