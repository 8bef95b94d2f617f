"""Exact-operand parity of every GEMM / conv route and epilogue form (docs/parity.md "Exact-operand parity of the contraction kernels").

Operands are small integers / dyadic fractions (tests/support/exact_contraction.py), so every fp32 partial sum is exact in any order: the fp32
output must have the BITS of the float64 reference, a bf16 output the bits of its round-to-nearest-even. Every case runs through
ir_op_linear_ex / ir_op_conv_ex (the host code of the product's launches) and asserts: the route ir_op_igemm_route reports and the profiler's
row; outputs, second output and V^T copy bit for bit; a second launch bit-equal; NaN-prefilled buffers fully written; canaries behind every
buffer and in every row's padding columns untouched. The forms with an inexact activation are gated at 8 x the deviation of an fp32 host
evaluation from float64 on the case's own pre-activations (+ 2^-9 relative for a bf16 output).

The first case (one k-tile, plain igemm_kernel) is the premise on its own: MFMA fp32 accumulation returns exact results for exact sums."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from instarevive_amd import _lib as L
from tests.support import exact_contraction as E

pytestmark = pytest.mark.gpu

CANARY = 4096
PAT32, PAT16 = 0x7FC0BEEF, 0x7FC1     # quiet NaNs: an element nobody wrote shows in the comparison, a canary somebody wrote in the bit check
_REFS = {}
_REFS_UNIVERSE = {}


def _ref(case):
    if case["name"] not in _REFS:
        _REFS.clear()     # one at a time: the gemm_pp references are 110 MB each
        ops = E.operands(case)
        _REFS[case["name"]] = (ops, E.reference(case, ops))
    return _REFS[case["name"]]


def _universe(ctx):
    if "universe" not in _REFS_UNIVERSE:
        _REFS_UNIVERSE["universe"] = E.route_universe(ctx.lib)
    return _REFS_UNIVERSE["universe"]


def _canvas(rows, cs, f32):
    """Host image of a buffer of rows x cs elements + CANARY behind, all NaN pattern (int32 / int16 view of the float data)."""
    return torch.full((rows * cs + CANARY,), PAT32 if f32 else PAT16, dtype=torch.int32 if f32 else torch.int16)


def _place(canvas, rows, cs, data_bits):
    canvas[:rows * cs].view(rows, cs)[:, :data_bits.shape[1]] = data_bits
    return canvas


def _bits(t, f32):
    return t.to(torch.float32).view(torch.int32) if f32 else t.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def _check_canary(buf, rows, cs, n, f32, what):
    pat = PAT32 if f32 else PAT16
    body = buf[:rows * cs].view(rows, cs)
    assert bool((buf[rows * cs:] == pat).all()), f"{what}: the canary behind the buffer was written"
    if cs > n:
        assert bool((body[:, n:] == pat).all()), f"{what}: padding columns {n} .. {cs - 1} were written"
    return body[:, :n]


def _compare(got_bits, ref, f32, tol, what):
    if tol == 0.0:
        want = _bits(ref, f32)
        absmask = 0x7FFFFFFF if f32 else 0x7FFF     # the sign of a zero is not compared (ReLU of a negative sum: x * 0 is -0 in IEEE, +0 with a select)
        got_bits = torch.where((got_bits & absmask) == 0, torch.zeros_like(got_bits), got_bits)
        want = torch.where((want & absmask) == 0, torch.zeros_like(want), want)
        if not torch.equal(got_bits, want):
            bad = (got_bits != want).nonzero()
            r, c = (int(v) for v in bad[0])
            view = (lambda b: b.view(torch.float32)) if f32 else (lambda b: b.view(torch.bfloat16).float())
            raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements differ from the float64 reference; first at row {r} column {c}: "
                                 f"got {float(view(got_bits)[r, c])!r}, reference {float(ref[r, c])!r}; rows {sorted(set(int(x) for x in bad[:, 0]))[:8]} ...")
        return
    got = (got_bits.view(torch.float32) if f32 else got_bits.view(torch.bfloat16).float()).double()
    if f32:
        lo, hi = ref - tol, ref + tol
    else:   # the value BEFORE the rounding may deviate by the gate + 2^-9 relative; the bf16 output is then the rounding of such a value (the
        # rounding itself moves a value by up to 2^-8 relative, so |got - ref| cannot be held to 2^-9)
        g = tol + 2.0 ** -9 * ref.abs()
        lo, hi = ((ref + s * g).float().to(torch.bfloat16).double() for s in (-1, 1))
    bad = ~((got >= lo) & (got <= hi))     # NaN fails
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside the activation gate {tol:.3g}, worst |got - ref| "
                           f"{float((got - ref).abs()[bad].max()):.3g} at reference {float(ref[bad][(got - ref).abs()[bad].argmax()]):.6g}")


def _device_args(case, ops):
    """Host-side images of every operand in the layouts the kernels read -> dict of CPU tensors (bit views)."""
    lin = case["kind"] == "linear"
    n_out, n_pad = case["cout"], case["cout_pad"]
    rows = E.rows_of(case)
    k = case["k"] if lin else case["cin"]
    in_cs = case["in_cs"] or k
    if lin:
        x = torch.full((case["m"], in_cs), 1000.0, dtype=torch.float64)   # padding columns nobody may read
        x[:, :k] = ops["x"]
        w = torch.zeros(n_pad, k, dtype=torch.float64)
        w[:n_out] = ops["w"]
    else:
        x = ops["x"].permute(0, 2, 3, 1).contiguous()
        w = E.pack_conv(ops["w"], n_pad)
    a = dict(x=L.bf16_bits(x.float()), w=L.bf16_bits(w.float()), wup=None, bias=None, gate=None, res=None, rows=rows)
    if case["phase"]:
        from instarevive_amd.weights import pack_conv_up2x2
        wp = torch.zeros(n_pad, *ops["w"].shape[1:])
        wp[:n_out] = ops["w"].float()
        a["wup"] = pack_conv_up2x2(wp)
    if ops["bias"] is not None:
        a["bias"] = torch.zeros(n_pad)
        a["bias"][:n_out] = ops["bias"].float()
    if ops["gate"] is not None:
        a["gate"] = torch.ones(n_pad)
        a["gate"][:n_out] = ops["gate"].float()
    if ops["res"] is not None:
        f32 = case["res"] == "f32"
        rr, cs = ops["res"].shape[0], case["res_cs"] or n_out
        a["res"] = _place(_canvas(rr, cs, f32), rr, cs, _bits(ops["res"], f32))
        a["res_rows"], a["res_cs"] = rr, cs
    return a


def _launch(ctx, case, a, route_only=False):
    """One launch into freshly prefilled buffers -> dict of the result buffers (CPU bit views) or the route."""
    lib = ctx.lib
    n_out, rows = case["cout"], a["rows"]
    f32 = bool(case["out_f32"])
    out_cs = case["out_cs"] or n_out
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else None) for k, v in a.items() if k in ("x", "w", "wup", "bias", "gate", "res")}
    out = dev["res"] if case["inplace"] else _canvas(rows, out_cs, f32).cuda()
    ex = L.IGemmEx()
    ex.in_cs, ex.out_cs, ex.res_cs, ex.res_mod = case["in_cs"], case["out_cs"], case["res_cs"], case["res_mod"]
    out2 = None
    out2_cs = case["out2_cs"] or n_out
    if case["out2"]:
        out2 = _canvas(rows, out2_cs, False).cuda()
        ex.out2, ex.out2_cs = out2.data_ptr(), case["out2_cs"]
    ex.splitk, ex.item_rows, ex.route_rows = int(case["splitk"]), case["item_rows"], case["route_rows"]
    ws = None
    if case["splitk"]:
        ws = torch.full((case["route"]["splits"] * rows * case["cout_pad"] + 1024,), float("nan"), device="cuda")
        ex.ws, ex.ws_bytes = ws.data_ptr(), ws.numel() * 4
    if dev["wup"] is not None:
        ex.wup = dev["wup"].data_ptr()
    vt = None
    if case["vt"]:
        v = case["vt"]
        heads = (n_out - v["col0"]) // v["hd"]
        vt = torch.full((v["batch"] * heads * v["dv"] * v["ld"] + CANARY,), PAT16, dtype=torch.int16).cuda()
        ex.vt_out, ex.vt_col0, ex.vt_hd, ex.vt_dv, ex.vt_ld, ex.vt_T, ex.vt_bs = vt.data_ptr(), v["col0"], v["hd"], v["dv"], v["ld"], v["T"], heads * v["dv"] * v["ld"]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    if case["kind"] == "linear":
        geom = (case["m"], 1, 1, case["k"], n_out, case["cout_pad"], 1, 1, 0, 0)
    else:
        geom = (case["n"], case["h"], case["w"], case["cin"], n_out, case["cout_pad"], 9, case["stride"], case["pad"], case["up"])
    tail = (case["act"], case["slope"], p(dev["res"]), int(case["res"] == "f32"), int(f32), p(dev["gate"]), float(case["out_scale"]), C.byref(ex))
    common = (ctx.h, ctx.stream(), p(dev["x"]), p(dev["w"]), p(dev["bias"]), p(out))
    if route_only:
        packed = int(lib.ir_op_igemm_route(*common, *geom, *tail))
        assert packed >= 0, f"ir_op_igemm_route refused: {packed}"
        return L.igemm_route_fields(packed)
    ctx.profile_begin()
    if case["kind"] == "linear":
        rc = lib.ir_op_linear_ex(*common, case["m"], case["k"], n_out, case["cout_pad"], case["act"], p(dev["gate"]), p(dev["res"]), int(case["res"] == "f32"),
                                 int(f32), float(case["out_scale"]), C.byref(ex))
    else:
        rc = lib.ir_op_conv_ex(*common, *geom, *tail)
    ctx.check(rc, case["name"])
    prof = ctx.profile_end_kernels()
    torch.cuda.synchronize()
    return dict(out=out.cpu(), out2=None if out2 is None else out2.cpu(), vt=None if vt is None else vt.cpu(), prof=prof, out_cs=out_cs, out2_cs=out2_cs)


@pytest.mark.parametrize("name", [c["name"] for c in E.CASES])
def test_exact(ctx, name):
    case = E.BY_NAME[name]
    ops, ref = _ref(case)
    a = _device_args(case, ops)
    n_out, rows, f32 = case["cout"], a["rows"], bool(case["out_f32"])
    ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1 if case["plain"] else 0), "ir_set_plain_kernels")
    try:
        route = _launch(ctx, case, a, route_only=True)
        want = case["route"]
        got_route = {k: route[k] for k in want}
        assert got_route == want, f"{name}: route {route}"
        assert E.route_key(route) in _universe(ctx), f"{name}: a route outside the range the library reports for its rule: {route}"
        r1 = _launch(ctx, case, a)
        r2 = _launch(ctx, case, a)
    finally:
        ctx.lib.ir_set_plain_kernels(ctx.h, 0)
    assert {k: v["launches"] for k, v in r1["prof"].items()} == {case["row"]: 1}, f"{name}: profiler rows {r1['prof']}"
    got = _check_canary(r1["out"], rows, r1["out_cs"], n_out, f32, f"{name} out")
    _compare(got, ref["out"], f32, ref["tol"], f"{name} out")
    assert torch.equal(r1["out"], r2["out"]), f"{name}: a second launch differs"
    if case["out2"]:
        got2 = _check_canary(r1["out2"], rows, r1["out2_cs"], n_out, False, f"{name} out2")
        _compare(got2, ref["out2"], False, ref["tol"], f"{name} out2")
        assert torch.equal(r1["out2"], r2["out2"]), f"{name}: out2 of a second launch differs"
    if case["vt"]:
        want_vt, mask = E.vt_reference(case, got)     # against the transposed bf16 OUTPUT (itself bit-equal to the reference above)
        body = r1["vt"][:want_vt.numel()].view(want_vt.shape)
        assert bool((r1["vt"][want_vt.numel():] == PAT16).all()), f"{name}: the canary behind V^T was written"
        assert torch.equal(body[mask], want_vt[mask]), f"{name}: V^T copy differs from the transposed output in {int((body[mask] != want_vt[mask]).sum())} elements"
        assert bool((body[~mask] == PAT16).all()), f"{name}: V^T rows d >= hd or columns t >= T were written"
        assert torch.equal(r1["vt"], r2["vt"])


def test_refusals_come_back_unchanged(ctx):
    """The launcher's refusal codes reach the caller of the new entries as they are, and nothing is written: Cin no multiple of 32 (-3), an in_cs
    below Cin (-3), Cout above Cout_pad (-4); a split-K workspace that is too small is -20 from the host layer."""
    case = dict(E.BY_NAME["lin_one_ktile"])
    ops, _ = _ref(case)
    a = _device_args(case, ops)
    x, w, b = a["x"].cuda(), a["w"].cuda(), a["bias"].cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(m, k, n, n_pad, **kw):
        out = _canvas(m, n, True).cuda()
        ex = L.IGemmEx()
        for key, v in kw.items():
            setattr(ex, key, v)
        rc = ctx.lib.ir_op_linear_ex(ctx.h, ctx.stream(), p(x), p(w), p(b), p(out), m, k, n, n_pad, 0, None, None, 0, 1, 1.0, C.byref(ex))
        torch.cuda.synchronize()
        assert bool((out.cpu() == PAT32).all()), "a refused launch wrote its output"
        return rc

    assert call(128, 48, 128, 128) == -3
    assert call(128, 64, 128, 128, in_cs=32) == -3
    assert call(128, 64, 128, 96) == -4
    ws = torch.zeros(1024, device="cuda")
    big = E.BY_NAME["lin_split3_k1536"]
    xb = torch.zeros(big["m"], big["k"], dtype=torch.int16, device="cuda")
    wb = torch.zeros(big["cout"], big["k"], dtype=torch.int16, device="cuda")
    out = _canvas(big["m"], big["cout"], True).cuda()
    ex = L.IGemmEx()
    ex.splitk, ex.ws, ex.ws_bytes = 1, ws.data_ptr(), 4096
    assert ctx.lib.ir_op_linear_ex(ctx.h, ctx.stream(), p(xb), p(wb), None, p(out), big["m"], big["k"], big["cout"], big["cout"], 0, None, None, 0, 1, 1.0, C.byref(ex)) == -20
    torch.cuda.synchronize()
    assert bool((out.cpu() == PAT32).all())


FP8_CASES = [
    # n, h, w, cin, cout, res, up, route (0 conv_halo_s1_fp8_kernel, 3 conv_halo_kernel<.., FP8>)
    (1, 16, 16, 128, 128, False, 0, 3),
    (2, 13, 21, 128, 64, True, 0, 3),       # 64-channel tiles, ragged 8 x 16 patches, two images
    (1, 64, 256, 128, 128, True, 0, 0),     # 32 patch tiles: the smallest map of the one-wave-per-SIMD kernel
    (2, 65, 225, 256, 128, False, 0, 0),    # ragged 16 x 32 patches, two periods
    (1, 9, 17, 128, 128, False, 1, 3),
    (1, 32, 128, 128, 128, False, 1, 0),
]


@pytest.mark.parametrize("n,h,w,cin,cout,res,up,route", FP8_CASES)
def test_exact_fp8(ctx, n, h, w, cin, cout, res, up, route):
    """e4m3 operands: integers up to 8 are exact in e4m3 and power-of-two dequantisation factors keep (acc + bias / f) * f + res exact, so
    ir_op_conv_fp8 / ir_op_conv_fp8_up give the bf16 rounding of the float64 result bit for bit on both fp8 conv kernels."""
    import numpy as np
    rng = np.random.default_rng(7000 + n + h + w + cin + cout + up)
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    assert ctx.lib.ir_op_conv_fp8_route(ctx.h, n, ho, wo, cin, cout, 1 if res else 0) == route
    x = torch.from_numpy(rng.integers(-3, 4, size=(n, cin, h, w)).astype(np.float64))
    wt = torch.from_numpy(rng.integers(-8, 9, size=(cout, cin, 3, 3)).astype(np.float64))
    deq = torch.from_numpy(np.exp2(rng.integers(-3, 1, size=cout).astype(np.float64)))
    bias = torch.from_numpy(rng.integers(-64, 65, size=cout).astype(np.float64))
    r_ = torch.from_numpy(rng.integers(-64, 65, size=(n * ho * wo, cout)).astype(np.float64)) if res else None
    assert torch.equal(x.to(torch.float8_e4m3fn).double(), x) and torch.equal(wt.to(torch.float8_e4m3fn).double(), wt)
    acc = E.conv_rows(x, wt, 1, 1, up)
    ref = (acc + bias / deq) * deq
    if res:
        ref = ref + r_
    assert float(9 * cin * 3 * 8 + 64 * 8) * 8 < E.LIMIT and torch.equal(ref.float().double(), ref)
    xin = x.permute(0, 2, 3, 1).contiguous().to(torch.float8_e4m3fn).view(torch.uint8).cuda()
    wp = wt.permute(0, 2, 3, 1).contiguous().to(torch.float8_e4m3fn).view(torch.uint8).cuda()
    deq_d, bias_d = deq.float().cuda(), (bias / deq).float().cuda()
    rd = _bits(r_, False).cuda() if res else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    outs = []
    for _ in range(2):
        out = _canvas(n * ho * wo, cout, False).cuda()
        ctx.profile_begin()
        if up:
            rc = ctx.lib.ir_op_conv_fp8_up(ctx.h, ctx.stream(), p(xin), p(wp), p(deq_d), p(bias_d), p(out), n, h, w, cin, cout)
        else:
            rc = ctx.lib.ir_op_conv_fp8(ctx.h, ctx.stream(), p(xin), p(wp), p(deq_d), p(bias_d), p(out), n, h, w, cin, cout, p(rd))
        ctx.check(rc, "conv_fp8")
        prof = ctx.profile_end_kernels()
        torch.cuda.synchronize()
        outs.append(out.cpu())
    row = "conv3x3/conv_halo_s1_fp8_kernel" if route == 0 else "conv3x3/conv_halo_kernel<.., fp8>"
    assert {k: v["launches"] for k, v in prof.items()} == {row: 1}, prof
    got = _check_canary(outs[0], n * ho * wo, cout, cout, False, "conv_fp8 out")
    _compare(got, ref, False, 0.0, f"conv_fp8 {(n, h, w, cin, cout, res, up)}")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n,h,w,cin,cout,res", [(1, 64, 256, 128, 128, True), (2, 65, 225, 256, 128, False)])
def test_exact_conv_norm(ctx, n, h, w, cin, cout, res):
    """conv_halo_s1_kernel's NORM form (ir_op_conv_norm: out = conv3x3(bf16(silu(in * scale + shift))) + res), made sharp: with integer in, scale
    1 or 2 and integer shifts of 23 .. 40 every a = in * scale + shift is an integer >= 17, where the kernel's silu(a) = a * rcp(1 + exp(-a)) IS a
    (exp(-17) < 2^-24) and the float64 SiLU rounds to a in bf16; a fifth of the channels get shift -200, where both give zero. The conv then
    sums integers, and the padding is zero AFTER the normalisation: a kernel that normalised its halo's padding (silu(shift) = shift) fails."""
    import numpy as np
    rng = np.random.default_rng(8000 + h + cin)
    x = torch.from_numpy(rng.integers(-3, 4, size=(n, cin, h, w)).astype(np.float64))
    wt = torch.from_numpy(E._ints(rng, cout, 9 * cin).reshape(cout, 3, 3, cin).transpose(0, 3, 1, 2).copy())
    scale = torch.from_numpy(rng.integers(1, 3, size=(n, cin)).astype(np.float64))
    shift = torch.from_numpy(np.where(rng.random((n, cin)) < 0.2, -200, rng.integers(23, 41, size=(n, cin))).astype(np.float64))
    bias = torch.from_numpy(rng.integers(-64, 65, size=cout).astype(np.float64))
    r_ = torch.from_numpy(rng.integers(-64, 65, size=(n * h * w, cout)).astype(np.float64)) if res else None
    a = x * scale[:, :, None, None] + shift[:, :, None, None]
    act = F.silu(a).float().to(torch.bfloat16).double()
    assert torch.equal(act, torch.where(a > 0, a, torch.zeros_like(a)))      # the sharpness argument above, checked
    ref = E.conv_rows(act, wt) + bias
    if res:
        ref = ref + r_
    assert 9 * cin * 46 * 3 + 128 < E.LIMIT and torch.equal(ref.float().double(), ref)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    xd = L.bf16_bits(x.permute(0, 2, 3, 1).contiguous().float()).cuda()
    wd = L.bf16_bits(E.pack_conv(wt, cout).float()).cuda()
    sc, sh, bd = scale.float().cuda(), shift.float().cuda(), bias.float().cuda()
    rd = _bits(r_, False).cuda() if res else None
    outs = []
    for _ in range(2):
        out = _canvas(n * h * w, cout, False).cuda()
        ctx.check(ctx.lib.ir_op_conv_norm(ctx.h, ctx.stream(), p(xd), p(sc), p(sh), p(wd), p(bd), p(rd), p(out), n, h, w, cin, cout), "conv_norm")
        torch.cuda.synchronize()
        outs.append(out.cpu())
    got = _check_canary(outs[0], n * h * w, cout, cout, False, "conv_norm out")
    _compare(got, ref, False, 0.0, f"conv_norm {(n, h, w, cin, cout, res)}")
    assert torch.equal(outs[0], outs[1])
