"""The bits of the six metric models, pinned: everything ir_lpips, ir_dists, ir_fid_features, ir_clipiqa, ir_musiq and ir_maniqa return for their
small cases against tests/golden/metric_bits_parent.json.

The gates of tests/test_{lpips,dists,fid,clipiqa,musiq,maniqa}_gpu.py are measured against float64 models and would not notice a change in
the last place. The six models share one exact-fp32 tile loop (csrc/exact_f32_tile.h), so this record is what tells a refactor of that loop, of
an operand policy or of an epilogue from a change of arithmetic. The comparison is of raw bits, no tolerance: an output of up to 64 bytes is
stored as the hex of its bytes, a larger one (features, moments, tokens, the resized image) as the SHA-256 of its bytes.

The cases are those of tests/support/*_model.py whose edges are both at most 131 pixels, plus fid's 300x301; they are run through the call
helpers of the six test modules. The file was recorded on the MI355X by `python -m tests.test_metric_bits_gpu --record`, which runs every case
twice and refuses to write an output that is not the same on both runs, from the library as it was before the six kernels were folded into the one
loop. It may be re-recorded only by a change that means to alter a model's arithmetic, and only from a build whose float64 gates (the six
modules above) pass; a change that does not mean to alter arithmetic and fails here has altered it."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from tests import test_clipiqa_gpu as TC
from tests import test_dists_gpu as TD
from tests import test_fid_gpu as TF
from tests import test_lpips_gpu as TL
from tests import test_maniqa_gpu as TA
from tests import test_musiq_gpu as TM
from tests.support import clipiqa_model as CM
from tests.support import dists_model as DM
from tests.support import fid_model as FM
from tests.support import lpips_model as LM
from tests.support import maniqa_model as AM
from tests.support import musiq_model as MM

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_bits_parent.json")
EDGE = 131
MODELS = ("lpips", "dists", "fid", "clipiqa", "musiq", "maniqa")


def _small(cases):
    """The cases (name, h, w, ..., weights, ...) with both edges at most EDGE, those of one weight binding together (a re-bind per binding)."""
    return sorted((c for c in cases if max(c[1], c[2]) <= EDGE), key=lambda c: [str(x) for x in c[3:5]])


def _pin(a):
    raw = np.ascontiguousarray(a).tobytes()
    return raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


def _lpips():
    out = {}
    for name, h, w, _, kind in sorted(_small(LM.CASES), key=lambda c: c[4] != "normal"):
        a, b = LM.pair(name)
        out[name] = {"score": _pin(TL._call(TL._tight([a]), TL._tight([b]), h, w, kind))}
    return out


def _dists():
    out = {}
    for name, h, w, _, kind in sorted(_small(DM.CASES), key=lambda c: c[4] != "normal"):
        a, b = DM.pair(name)
        s, m = TD._call(TD._tight([a]), TD._tight([b]), h, w, kind)
        out[name] = {"score": _pin(s), "moments": _pin(m)}
    return out


def _fid():
    out = {}
    for name in [n for n, c in FM.CASES.items() if max(c[0], c[1]) <= EDGE] + ["300x301"]:
        f, b, r = TF._call([FM.image(name)], FM.CASES[name][3])
        out[name] = {"features": _pin(f), "block_means": _pin(b), "resized": _pin(r)}
    return out


def _clipiqa():
    out = {}
    for name, h, w, kind in _small(CM.CASES):
        s, f = TC._call(TC._tight([CM.image(name)]), h, w, kind)
        out[name] = {"score": _pin(s), "features": _pin(f)}
    return out


def _musiq():
    out = {}
    for name, h, w, kind in _small(MM.CASES):
        s, f = TM._call(TM._tight([MM.image(name)]), h, w, kind)
        out[name] = {"score": _pin(s), "features": _pin(f)}
    return out


def _maniqa():
    out = {}
    for name, h, w, kind, _, _ in _small(AM.CASES):
        s, f = TA._call(TA._tight([AM.image(name)]), h, w, [AM.origins(name)], kind)
        out[name] = {"score": _pin(s), "tokens": _pin(f)}
    return out


RUN = dict(lpips=_lpips, dists=_dists, fid=_fid, clipiqa=_clipiqa, musiq=_musiq, maniqa=_maniqa)


@pytest.mark.parametrize("model", MODELS)
def test_every_output_has_the_recorded_bits(model):
    with open(GOLDEN) as fh:
        want = json.load(fh)[model]
    got = RUN[model]()
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    assert all(sorted(got[c]) == sorted(want[c]) for c in got)
    bad = [(case, k) for case in got for k in got[case] if got[case][k] != want[case][k]]
    assert not bad, f"{model}: outputs whose bits differ from the record: {bad}"


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and len(sys.argv) <= 3, "usage: python -m tests.test_metric_bits_gpu --record [FILE]"
    record = {}
    for model in MODELS:
        first, second = RUN[model](), RUN[model]()
        unstable = [(c, k) for c in first for k in first[c] if first[c][k] != second[c][k]]
        assert not unstable, f"{model}: not the same bits on two runs: {unstable}"
        record[model] = first
        print(model, {c: sorted(v) for c, v in first.items()}, flush=True)
    with open(sys.argv[2] if len(sys.argv) == 3 else GOLDEN, "w") as fh:
        json.dump(record, fh, indent=1, sort_keys=True)
        fh.write("\n")
