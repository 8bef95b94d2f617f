"""CPU half of the exact-operand parity of the GEMM / conv kernels (tests/support/exact_contraction.py, docs/parity.md "Exact-operand parity of
the contraction kernels"): the premise holds for every case of the table, the table reaches every route the query can report, every planted bug
changes its case, and the recorded justification - what the tolerances of test_linear and test_conv3x3 let through."""
import math

import pytest
import torch

from tests.support import exact_contraction as E

_REFS = {}


def _ref(name):
    if name not in _REFS:
        case = E.BY_NAME[name]
        ops = E.operands(case)
        acc = E.contraction(case, ops)
        E.check_premise(case, ops, acc)
        _REFS[name] = (ops, acc, E.reference(case, ops, acc=acc))
    return _REFS[name]


@pytest.mark.parametrize("name", [c["name"] for c in E.CASES])
def test_premise(name):
    """Per case: the largest possible |partial sum| is below 2^24 units, the float64 contraction and every epilogue value of an exact form equal
    their own fp32 rounding, for K >= 4096 at least half the sums exceed 2^9 (all asserted inside the module), rows and columns have means of
    their own, and the fp32 host evaluation of an inexact activation gives a finite, small gate."""
    case = E.BY_NAME[name]
    ops, acc, ref = _ref(name)
    x = ops["x"] if case["kind"] == "linear" else ops["x"].permute(0, 2, 3, 1).reshape(-1, case["cin"])
    w = ops["w"].reshape(case["cout"], -1)
    assert float(x.abs().max()) <= 3 and float(w.abs().max()) <= 3
    assert torch.equal(x.to(torch.bfloat16).double(), x) and torch.equal(w.to(torch.bfloat16).double(), w)
    for t in (x, w):
        if not case["eighths"]:
            sums = t.sum(dim=1)
            assert float(sums.abs().min()) > 0 and (len(sums) < 2 or bool((sums[1:] != sums[:-1]).all()))   # a swapped neighbour shows
    if E.exact_act(case):
        assert ref["tol"] == 0.0
        assert torch.equal(ref["out"].float().double(), ref["out"])
    else:
        assert 0.0 < ref["tol"] < 2e-3, ref["tol"]   # 8 x an fp32 rounding of values up to a few hundred
    if case["res"] == "bf16":
        assert torch.equal(ops["res"].to(torch.bfloat16).double(), ops["res"])


def _lib_loaded():
    from instarevive_amd import _lib
    from instarevive_amd.build import build
    build()
    return _lib.load_library()


def test_case_table_reaches_every_route():
    """The universe is not a list kept here: the library evaluates its own rule over a grid of launches (ir_op_igemm_route_range)."""
    universe = E.route_universe(_lib_loaded())
    assert {k[0] for k in universe} >= {0, 1, 2, 3, 4} and {k[6] for k in universe} == {1, 9}
    reached = E.check_complete(universe)
    assert set(E.UNREACHED_ALLOWED) == {(5, 0, 0, 0, 0, 0, 9)}       # conv64 and nothing else
    assert not (reached & set(E.UNREACHED_ALLOWED))
    assert E.CASES[0]["name"] == "lin_one_ktile_plain"               # the premise case runs first on the GPU
    one = [c for c in E.CASES if c["kind"] == "linear" and c["k"] == 64 and c["plain"]]
    assert one and one[0]["route"]["stages"] == 2
    ms = {c["m"] for c in E.CASES if c["kind"] == "linear" and c["route"]["kernel"] == 4}
    assert {1, 127, 128, 129, 260} <= ms
    ks = {c["k"] for c in E.CASES if c["kind"] == "linear" and c["route"]["kernel"] == 4}
    assert {32, 96, 64, 448, 512, 4608} <= ks
    assert {c["route"]["form"] for c in E.CASES if c["route"]["kernel"] == 2} == {0, 1, 2, 3}
    # gemm_pp_kernel at exactly its shortest reduction (8 of its 32-wide k-tiles), every form, and at a longer one; one k-tile below: generic
    assert E.PP_MIN_K == 256
    assert {c["route"]["form"] for c in E.CASES if c["route"]["kernel"] == 2 and c["k"] == E.PP_MIN_K} == {0, 1, 2, 3}
    assert {c["route"]["form"] for c in E.CASES if c["route"]["kernel"] == 2 and c["k"] > E.PP_MIN_K} == {0, 1, 2, 3}
    assert any(c["vt"] and c["k"] == E.PP_MIN_K for c in E.CASES)
    below = E.BY_NAME["pp_k224_below_min_k"]
    assert below["k"] == E.PP_MIN_K - E.PP_BK and below["route"]["kernel"] == 4 and below["m"] == E.PP_M


@pytest.mark.parametrize("bug", sorted(E.BUGS))
def test_planted_bug_changes_its_case(bug):
    case = E.BY_NAME[E.BUGS[bug]]
    ops, acc, ref = _ref(case["name"])
    if bug == "vt_head_tail":
        bits = ref["out"].to(torch.bfloat16).view(torch.int16)
        vt, mask = E.vt_reference(case, bits)
        bad = E.plant_vt(case, vt, mask)
        assert int((bad != vt)[mask].sum()) > 0
        return
    got = E.reference(case, ops, bug=bug, acc=acc)
    changed = int((got["out"] != ref["out"]).sum())
    if bug == "out2_before_res":
        changed = int((got["out2"] != ref["out2"]).sum())
    assert changed > 0, f"{bug} leaves {case['name']} unchanged"
    # ... and the changed elements are wrong after rounding to the output format too (what the GPU test compares)
    if bug != "out2_before_res":
        fmt = torch.float32 if case["out_f32"] else torch.bfloat16
        assert int((got["out"].float().to(fmt) != ref["out"].float().to(fmt)).sum()) > 0


def test_new_entries_are_exported_and_refuse_a_null_context():
    """ir_op_linear_ex / ir_op_conv_ex / ir_op_igemm_route: declared, exported, additive (the ABI version stays), and -1 before any device call for
    a null context or a null ir_igemm_ex."""
    import ctypes as C
    from instarevive_amd import _lib
    from instarevive_amd.build import build
    build()
    lib = _lib.load_library()
    assert lib.ir_abi_version() == 3
    ex = _lib.IGemmEx()
    for name in ("ir_op_linear_ex", "ir_op_conv_ex", "ir_op_igemm_route"):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        args = [0.0 if t is C.c_float else 0 if t is C.c_int else None for t in fn.argtypes]
        assert fn(*args) == -1, name
        assert fn(*args[:-1], C.byref(ex)) == -1, name
    f = _lib.igemm_route_fields((4 | 0 << 4 | 1 << 7 | (128 // 4) << 8 | (64 // 16) << 16 | 4 << 20 | 8 << 24 | 9 << 28 | 15 << 32 | 1 << 40 | 1 << 41))
    assert f == dict(kernel=4, form=0, vt=1, bn=128, bk=64, stages=4, waves=8, taps=9, splits=15, padded=1, idle=1, fp8=0)


def _inside(delta, ref, rtol, atol):
    """Of the elements a bug changes: how many stay inside |err| <= atol + rtol |ref| (close() of tests/test_ops_gpu.py), and whether all do."""
    hit = delta != 0
    ok = (delta.abs() <= atol + rtol * ref.abs()) & hit
    return int(ok.sum()), int(hit.sum())


def test_old_tolerances_let_planted_bugs_through():
    """The recorded justification. On the random-normal data and with the tolerances of test_linear (atol 2e-4 sqrt(k), rtol 1e-4 on fp32 output)
    a lost or doubled TERM of a long reduction moves an output by about the tolerance. Measured at (2100, 4608, 256): 9902 of the 13312 elements
    of the ragged tile that lose their last k element stay inside the tolerance (74 %), 78 % of the elements with one k element added twice
    (the planted bug double_k_element), 9 % of those with a whole 64-element k-tile added twice (double_ktile); at (1000, 1152, 64) 32 %, 40 %
    and 2 %. close() wants EVERY element inside, so a bug that
    hits thousands of elements is still caught through its tail and the literal 'the bug passes close()' does not hold for such a bug; what
    holds, and is asserted, is the per-element figure: a kernel that goes wrong in a FEW elements of a long reduction more likely passes than
    not. test_conv3x3's tolerance (atol 1e-3 on fp32 output, K <= 1152) is tight against a whole misplaced halo PIXEL (cin terms, |delta|
    about 1/3): at most 1 % of the changed elements pass, that bug is caught there. The conv kernels' gap is the bf16-output gates (2^-7
    relative) and the block-level relative-L2 gates, not test_conv3x3.
    The exact operands catch every changed element of every planted bug (test_planted_bug_changes_its_case)."""
    from tests import test_ops_gpu as T
    shapes = T.test_linear.pytestmark[0].args[1]
    best = {"drop_last_k_ragged_m": 0.0, "double_k_element": 0.0, "double_ktile": 0.0}
    literal = {b: False for b in best}     # does close() - EVERY element inside - pass the planted bug on some shape of test_linear?
    for m, k, n in shapes:
        g = torch.Generator().manual_seed(m + k + n)
        x = T.rb(torch.randn(m, k, generator=g))
        w = T.rb(torch.randn(n, k, generator=g) / math.sqrt(k))
        b = torch.randn(n, generator=g)
        ref = x @ w.t() + b
        d1 = E.delta_drop_last_k(x, w)
        # the planted bugs of BUGS themselves: a doubled k ELEMENT (the smallest form of "one k-tile added twice") and the whole 64-element tile
        d2 = E.delta_double_k_element(x, w)
        d3 = E.delta_double_ktile(x, w)
        for bug, d in (("drop_last_k_ragged_m", d1), ("double_k_element", d2), ("double_ktile", d3)):
            ok, hit = _inside(d, ref.double(), 1e-4, 2e-4 * math.sqrt(k))
            if hit:
                best[bug] = max(best[bug], ok / hit)
                literal[bug] = literal[bug] or ok == hit
    assert best["drop_last_k_ragged_m"] > 0.5, best    # (2100, 4608, 256): more than half of the wrong elements pass
    assert best["double_k_element"] > 0.5, best
    assert best["double_ktile"] < 0.5, best            # a whole tile is 64 terms: mostly outside
    # recorded, not wished for: none of them passes close() as a whole - each changes thousands of elements, and the tail of those is outside
    assert literal == {"drop_last_k_ragged_m": False, "double_k_element": False, "double_ktile": False}, literal
    # conv: one halo pixel from the neighbouring row at the right border
    shares = []
    for case in T.CONV_CASES:
        n, h, wd, cin, cout, stride, pad, up = case
        if stride != 1 or up:
            continue
        g = torch.Generator().manual_seed(sum(case))
        x = T.rb(torch.randn(n, cin, h, wd, generator=g))
        wt = T.rb(torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin))
        b = torch.randn(cout, generator=g)
        ref = torch.nn.functional.conv2d(x, wt, b, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
        ok, hit = _inside(E.delta_halo_wrap(x, wt), ref.double(), 1e-4, 1e-3)
        shares.append(ok / hit)
    assert max(shares) < 0.05, shares   # test_conv3x3 does catch this one: recorded, see the docstring
