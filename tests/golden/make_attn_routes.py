"""Record tests/golden/attn_routes.json: per case of tests/test_attn_routes_gpu.py the SHA-256 of the output bytes and the launches per
profiler row, on the MI355X. The library under test is the one INSTAREVIVE_HIP_LIB names (a build of the commit whose behaviour is to be
pinned), else the tree's own.

    INSTAREVIVE_HIP_LIB=/path/to/libinstarevive_hip.so python tests/golden/make_attn_routes.py [output.json [case ...]]

With case names only those are recorded, into what tests/golden/attn_routes.json already holds.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_attn_routes_gpu as T  # noqa: E402


class Fixtures:
    """What the cases ask of pytest's `request`: the session fixtures of tests/conftest.py, built the same way."""

    def __init__(self):
        self.made = {}

    def getfixturevalue(self, name):
        if name not in self.made:
            self.made[name] = getattr(self, "_" + name)()
        return self.made[name]

    def _ctx(self):
        from instarevive_amd import Context
        return Context(0)

    def _full_models(self):
        import bench
        swin, vae, dit, _sched, sds = bench.build_models(torch.device("cuda", 0), lambda m: None)
        y, mask = bench.synthetic_prompt()

        class Full(tuple):
            pass

        full = Full((swin, vae, dit, sds, y, mask))
        full.y_cuda, full.mask_cuda = y.cuda(), mask.cuda()
        return full


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    req = Fixtures()
    only = sys.argv[2:]
    cases = {k: v for k, v in T.golden()["cases"].items() if k in T.CASES} if only else {}
    for name in only or T.CASES:
        cases[name] = T.record(name, req)
        print(name, cases[name], flush=True)
    with open(out, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
