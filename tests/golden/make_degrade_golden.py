"""Generate tests/golden/degrade.npz by RUNNING THE REFERENCE's own utils/degradation.py (imported read-only) on fixed arguments:

    python tests/golden/make_degrade_golden.py --reference REFERENCE_ROOT

Nothing from the reference is copied: the fixture holds arrays only - the arguments and outputs of bivariate_Gaussian for six
(K, sig_x, sig_y, theta, isotropic) cases and of add_gaussian_noise (clip=True) on a fixed image with numpy's global generator seeded, together
with the standard-normal field that seed gives. cv2 and torchvision.transforms.functional_tensor, which the module imports and these two
functions never call, are stubbed as SURVEY.md appendix A describes.
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(41, 0.1, 0.1, 0.0, True), (41, 10.0, 10.0, 0.0, True), (41, 3.7, 0.6, 0.9, False), (41, 0.1, 10.0, -2.5, False),
         (21, 2.25, 5.5, 3.0, False), (7, 1.3, 1.3, 0.0, True)]
NOISE_SEED, NOISE_SIGMA, NOISE_SHAPE = 4321, 12.5, (9, 11, 3)


def import_degradation(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)

    def mk(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m
    mk("cv2")
    for name in ("torchvision", "torchvision.transforms"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                mk(name)
    mk("torchvision.transforms.functional_tensor", rgb_to_grayscale=None)
    from utils import degradation
    return degradation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (read only)")
    ap.add_argument("--out", default=os.path.join(HERE, "degrade.npz"))
    a = ap.parse_args()
    D = import_degradation(os.path.abspath(a.reference))
    out = {"cases": np.array(CASES, dtype=np.float64)}
    for i, (K, sx, sy, th, iso) in enumerate(CASES):
        k = D.bivariate_Gaussian(K, sx, sy, th, isotropic=bool(iso))
        assert k.dtype == np.float64 and k.shape == (K, K)
        out[f"kernel_{i}"] = k
    img = (np.random.default_rng(7).integers(0, 256, NOISE_SHAPE) / 255.0).astype(np.float32)
    np.random.seed(NOISE_SEED)
    field = np.float32(np.random.randn(*NOISE_SHAPE))
    np.random.seed(NOISE_SEED)
    noisy = D.add_gaussian_noise(img, sigma=NOISE_SIGMA, clip=True)
    assert noisy.dtype == np.float32
    out.update(noise_img=img, noise_field=field, noise_sigma=np.float64(NOISE_SIGMA), noise_out=noisy)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
