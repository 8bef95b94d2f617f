"""Exact-operand parity of the GEMM / conv kernels: operands, float64 reference, planted bugs and the case table (plain numpy / torch, no GPU).

The idea: with operands that are small integers (or dyadic fractions) every product and every partial sum of a contraction is exactly
representable in fp32 as long as |sum| < 2^24 units, so fp32 accumulation gives ONE result whatever the order, the tile shape or the split -
the float64 result, bit for bit. A lost, doubled or misplaced term is then a wrong integer, not noise, and no tolerance is needed.

  operands(case)             seeded x, w (integers in [-3, 3], x in eighths for `eighths` cases; every row of x and every output column of w with
                             a mean of its own), bias / residual / periodic table (integers in [-64, 64]), gate / out_scale (powers of two)
  reference(case, ops, bug)  float64, epilogue in igemm_epilogue's order: act(acc + bias) * out_scale * gate + res; checks the premise per case
  BUGS                       planted bugs, applied to the reference
  CASES                      the case table of tests/test_contraction_exact_gpu.py with the route each case must take
  route_universe(lib)        every route the query can report for bf16 operands, from the library's own rule (ir_op_igemm_route_range);
                             check_complete() holds CASES against it
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU_ERF, ACT_GELU_TANH, ACT_LRELU, ACT_SILU = range(5)
BM = 128            # row tile of igemm_kernel
PP_BM, PP_BN, PP_BK = 256, 288, 32   # tile and k-tile of gemm_pp_kernel (GemmPP in csrc/igemm.hip)
PP_MIN_K = 8 * PP_BK      # GEMM_PP_MIN_K: the shortest reduction gemm_pp_kernel takes, 8 of ITS k-tiles
LIMIT = float(2 ** 24)


# ------------------------------------------------------------------------------------------------------------------------ operands
def _ints(rng, rows, cols):
    """[rows][cols] integers in [-3, 3]; row r is shifted by -2, -1, 1 or 2 (clipped) on a share of its elements that differs from row to row, so
    every row has a non-zero mean of its own and a swapped row shows."""
    u = rng.integers(-3, 4, size=(rows, cols))
    shift = rng.choice(np.array([-2, -1, 1, 2]), size=(rows, 1))
    share = ((np.arange(rows) * 0.6180339887 + 0.25) % 1.0)[:, None] * 0.8 + 0.2
    take = rng.random((rows, cols)) < share
    a = np.where(take, np.clip(u + shift, -3, 3), u)
    sums = a.sum(axis=1)
    for r in range(rows):   # chance can still cancel a short row's mean or repeat its neighbour's: move one element until it does neither
        c = r % cols
        while sums[r] == 0 or (r > 0 and sums[r] == sums[r - 1]):
            step = 1 if a[r, c] < 3 else -1
            a[r, c] += step
            sums[r] += step
            c = (c + 1) % cols
    return a.astype(np.float64)


def _pow2(rng, size, lo=-2, hi=2):
    return np.exp2(rng.integers(lo, hi + 1, size=size).astype(np.float64))


def out_hw(case):
    if case["kind"] == "linear":
        return 1, 1
    h, w = case["h"], case["w"]
    if case["stride"] == 2:
        return h // 2, w // 2
    return (2 * h, 2 * w) if case["up"] else (h, w)


def rows_of(case):
    if case["kind"] == "linear":
        return case["m"]
    ho, wo = out_hw(case)
    return case["n"] * ho * wo


def operands(case):
    """-> dict of float64 torch tensors: x ([m][k] or NCHW), w ([n][k] or [cout][cin][3][3]), bias [cout], gate [cout] or None, res ([rows or
    res_mod][cout]) or None, and out_scale (float)."""
    rng = np.random.default_rng(case["seed"])
    n_out = case["cout"]
    if case["kind"] == "linear":
        x = _ints(rng, case["m"], case["k"])
        w = _ints(rng, n_out, case["k"])
    else:
        n, h, wd, cin = case["n"], case["h"], case["w"], case["cin"]
        x = _ints(rng, n * h * wd, cin).reshape(n, h, wd, cin).transpose(0, 3, 1, 2).copy()           # a pixel is a row of the implicit GEMM
        w = _ints(rng, n_out, 9 * cin).reshape(n_out, 3, 3, cin).transpose(0, 3, 1, 2).copy()
    if case["eighths"]:
        x = np.clip(x * 8 + rng.integers(-7, 8, size=x.shape), -24, 24) / 8.0
    ops = dict(x=torch.from_numpy(x), w=torch.from_numpy(w), gate=None, res=None, out_scale=float(case["out_scale"]))
    ops["bias"] = torch.from_numpy(rng.integers(-64, 65, size=n_out).astype(np.float64)) if case["bias"] else None
    if case["gate"]:
        ops["gate"] = torch.from_numpy(_pow2(rng, n_out))
    if case["res"]:
        rr = case["res_mod"] if case["res_mod"] else rows_of(case)
        ops["res"] = torch.from_numpy(rng.integers(-64, 65, size=(rr, n_out)).astype(np.float64))
    return ops


# ------------------------------------------------------------------------------------------------------------------------ reference
def pack_conv(w, cout_pad):
    """[cout][cin][3][3] -> [cout_pad][9 * cin] (tap-major, channel-minor), the layout the conv kernels read."""
    co, ci = w.shape[:2]
    p = torch.zeros(cout_pad, 9 * ci, dtype=w.dtype)
    p[:co] = w.permute(0, 2, 3, 1).reshape(co, 9 * ci)
    return p


def conv_rows(x, w, stride=1, pad=1, up=0):
    """float64 conv2d as the kernels define it -> [n * ho * wo][cout] (NHWC rows). stride 2: pad (0, 1, 0, 1); up: nearest 2x first."""
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    y = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, None, stride=2) if stride == 2 else F.conv2d(xin, w, None, padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def conv_rows_phase(x, wup):
    """The same nearest-2x + 3x3 conv from the packed phase weights of weights.pack_conv_up2x2 ([4 phases][cout][4 taps][cin]): output pixel
    (2y + dy, 2x + dx) = sum over (sy, sx) of wup[2 dy + dx][:, 2 sy + sx] . x[y - 1 + dy + sy, x - 1 + dx + sx]."""
    n, ci, h, w = x.shape
    co = wup.shape[0] // 4
    k = wup.view(torch.bfloat16).to(torch.float64).reshape(4, co, 2, 2, ci).permute(0, 1, 4, 2, 3)   # wup: bf16 bits (int16)
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros(n, co, 2 * h, 2 * w, dtype=torch.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            y[:, :, dy::2, dx::2] = F.conv2d(xp[:, :, dy:dy + h + 1, dx:dx + w + 1], k[2 * dy + dx].contiguous())
    return y.permute(0, 2, 3, 1).reshape(-1, co)


def contraction(case, ops):
    if case["kind"] == "linear":
        return ops["x"] @ ops["w"].t()
    acc = conv_rows(ops["x"], ops["w"], case["stride"], case["pad"], case["up"])
    if case["phase"]:
        from instarevive_amd.weights import pack_conv_up2x2
        wup = pack_conv_up2x2(ops["w"].float())
        assert torch.equal(conv_rows_phase(ops["x"], wup), acc), f"{case['name']}: the phase weights do not compute the nearest-2x conv"
    return acc


def act64(pre, act, slope):
    if act == ACT_GELU_ERF:
        return F.gelu(pre)
    if act == ACT_GELU_TANH:
        return F.gelu(pre, approximate="tanh")
    if act == ACT_LRELU:
        return torch.where(pre > 0, pre, pre * slope)
    if act == ACT_SILU:
        return F.silu(pre)
    return pre


def exact_act(case):
    """Forms whose whole epilogue is exact: no activation, or LeakyReLU with a power-of-two slope (a linear has no slope argument: slope 0, ReLU)."""
    return case["act"] == ACT_NONE or (case["act"] == ACT_LRELU and (case["slope"] == 0.0 or math.log2(case["slope"]).is_integer()))


def _fp32_exact(t):
    return torch.equal(t.to(torch.float32).to(torch.float64), t)


def check_premise(case, ops, acc):
    """What makes the comparison exact, per case: the largest possible |partial sum| stays below 2^24 units (the unit is the operands' smallest
    dyadic step), and for K >= 4096 at least half the sums exceed 2^9, so that an accumulator narrower than fp32 cannot pass."""
    x, w = ops["x"], ops["w"]
    unit = 8.0 if case["eighths"] else 1.0
    if case["kind"] == "linear":
        bound = float((x.abs().sum(dim=1).max()) * w.abs().max())
        K = case["k"]
    else:   # a window covers at most 9 pixels (18 with the upsample's repeats counted once each: still 9 taps) of all channels
        bound = float(9 * x.abs().sum(dim=1).max() * w.abs().max())
        K = 9 * case["cin"]
    extra = 64.0 * (1 if case["bias"] else 0) + 64.0 * (1 if case["res"] else 0)
    scale_up = 16.0 if (case["gate"] or case["out_scale"] != 1.0) else 1.0   # gate * out_scale moves the binary point by at most 4 places either way
    assert (bound + extra) * unit * scale_up < LIMIT, f"{case['name']}: a partial sum could reach {bound + extra} x {unit * scale_up} >= 2^24"
    assert _fp32_exact(acc), f"{case['name']}: the float64 contraction is not its own fp32 rounding"
    if K >= 4096:
        share = float((acc.abs() > 512).double().mean())
        assert share >= 0.5, f"{case['name']}: only {share:.2f} of the sums exceed 2^9"


def reference(case, ops, bug=None, acc=None):
    """-> dict(out=float64 [rows][cout], out2=float64 or None, pre=the pre-activations, tol=absolute gate of an activation form (0: exact)).
    bug: a name of BUGS, applied on the way (see plant())."""
    if acc is None:
        acc = contraction(case, ops)
        if bug is None:
            check_premise(case, ops, acc)
    if bug in _ACC_BUGS:
        acc = acc + _ACC_BUGS[bug](case, ops)
    pre = acc if ops["bias"] is None else acc + ops["bias"]
    a = act64(pre, case["act"], case["slope"])
    gate = ops["gate"]
    if bug == "gate_shift4" and gate is not None:
        gate = torch.roll(gate, 4)
    v = a * ops["out_scale"]
    if gate is not None:
        v = v * gate
    if bug == "bias_twice" and ops["bias"] is not None:
        v = v + ops["bias"]
    before_res = v
    if ops["res"] is not None:
        rows = torch.arange(acc.shape[0])
        if case["res_mod"]:
            rows = rows % case["res_mod"] if bug != "res_mod_ignored" else torch.clamp(rows, max=case["res_mod"] - 1)
        if bug == "res_row_plus1":
            rows = (rows + 1) % ops["res"].shape[0]
        v = v + ops["res"][rows]
    out2 = None
    if case["out2"]:
        out2 = before_res if bug == "out2_before_res" else v
    if bug == "idle_block_rewrites_tile0":   # the padding block computed nothing: tile 0 holds what its (empty) accumulators give
        bn = case["route"]["bn"]
        v = v.clone()
        v[:BM, :bn] = (v - acc * (ops["out_scale"] * (gate if gate is not None else 1.0)))[:BM, :bn]
    tol = 0.0
    if not exact_act(case):
        # the exact pre-activation is known; what an fp32 evaluation of the activation may deviate by is MEASURED on this case's own
        # pre-activations with torch's fp32 CPU kernels (never with the library's result), times 8
        dev = (act64(pre.to(torch.float32), case["act"], case["slope"]).to(torch.float64) - a).abs().max()
        tol = 8.0 * float(dev) * abs(ops["out_scale"]) * (float(gate.abs().max()) if gate is not None else 1.0)
    elif bug is None:
        assert _fp32_exact(pre) and _fp32_exact(before_res) and _fp32_exact(v), f"{case['name']}: an epilogue value is not exact in fp32"
    return dict(out=v, out2=out2, pre=pre, tol=tol)


def vt_reference(case, out_bits):
    """The transposed copy the launch must write next to its bf16 output (IGemmParams::vt_out): from the OUTPUT's bf16 bits [m][n] (int16) ->
    [batch][head * dv + d][ld] with only d < hd, t < T written (None elsewhere: a mask says which elements)."""
    vt = case["vt"]
    b, T, hd, dv, ld, col0 = vt["batch"], vt["T"], vt["hd"], vt["dv"], vt["ld"], vt["col0"]
    heads = (case["cout"] - col0) // hd
    v = out_bits[:, col0:].reshape(b, T, heads, hd).permute(0, 2, 3, 1)          # [b][head][d][t]
    ref = torch.zeros(b, heads, dv, ld, dtype=out_bits.dtype)
    mask = torch.zeros(b, heads, dv, ld, dtype=torch.bool)
    ref[:, :, :hd, :T] = v
    mask[:, :, :hd, :T] = True
    return ref.reshape(b, heads * dv, ld), mask.reshape(b, heads * dv, ld)


# ------------------------------------------------------------------------------------------------------------------------ planted bugs
def delta_drop_last_k(x, w, m_tile=BM):
    """linear: the last k element is lost for the rows of the ragged last M tile."""
    m = x.shape[0]
    d = torch.zeros(m, w.shape[0], dtype=torch.float64)
    r0 = (m // m_tile) * m_tile
    if r0 < m:
        d[r0:] = -x[r0:, -1:].double() * w[:, -1].double()[None, :]
    return d


def delta_double_ktile(x, w, bn=128, bk=64):
    """linear: k-tile 0 is added twice for column tile 0."""
    d = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64)
    d[:, :bn] = x[:, :bk].double() @ w[:bn, :bk].double().t()
    return d


def delta_double_k_element(x, w, bn=128):
    """linear: ONE k element (the smallest k-tile a kernel could have) is added twice for column tile 0 - the few-term form of double_ktile,
    the one the old tolerances are measured against in tests/test_contraction_exact_cpu.py."""
    d = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64)
    d[:, :bn] = x[:, :1].double() * w[:bn, 0].double()[None, :]
    return d


def delta_halo_wrap(x, w, y0=0):
    """conv (stride 1, pad 1): at the right image border of row y0 the halo pixel (y0, W) - padding - is read from the next address, (y0 + 1, 0)."""
    n, ci, h, wd = x.shape
    d = torch.zeros(n, h, wd, w.shape[0], dtype=torch.float64)
    d[:, y0, wd - 1] = x[:, :, y0 + 1, 0].double() @ w[:, :, 1, 2].double().t()
    return d.reshape(-1, w.shape[0])


def delta_replicate_corner(x, w):
    """conv (stride 1, pad 1): the zero padding above and left of pixel (0, 0) is replaced by that pixel."""
    n, ci, h, wd = x.shape
    d = torch.zeros(n, h, wd, w.shape[0], dtype=torch.float64)
    d[:, 0, 0] = x[:, :, 0, 0].double() @ w[:, :, 0, 0].double().t()
    return d.reshape(-1, w.shape[0])


def delta_split_slice(case, ops):
    """split-K: slice 1 of the k-tiles is left out of the sum."""
    splits = case["route"]["splits"]
    if case["kind"] == "linear":
        kt = case["k"] // 64
        per = -(-kt // splits)
        k0, k1 = per * 64, min(2 * per, kt) * 64
        return -(ops["x"][:, k0:k1] @ ops["w"][:, k0:k1].t())
    cin = case["cin"]
    kt = 9 * cin // 64
    per = -(-kt // splits)
    wp = pack_conv(ops["w"], case["cout"]).clone()      # k runs tap-major, channel-minor
    keep = torch.zeros(9 * cin, dtype=torch.bool)
    keep[per * 64:min(2 * per, kt) * 64] = True
    wp[:, ~keep] = 0
    wz = wp.reshape(case["cout"], 3, 3, cin).permute(0, 3, 1, 2).contiguous()
    return -conv_rows(ops["x"], wz, case["stride"], case["pad"], case["up"])


_ACC_BUGS = {
    "drop_last_k_ragged_m": lambda case, ops: delta_drop_last_k(ops["x"], ops["w"]),
    "double_ktile": lambda case, ops: delta_double_ktile(ops["x"], ops["w"], case["route"]["bn"]),
    "double_k_element": lambda case, ops: delta_double_k_element(ops["x"], ops["w"], case["route"]["bn"]),
    "halo_wraps_at_right_border": lambda case, ops: delta_halo_wrap(ops["x"], ops["w"]),
    "replicate_pad_corner": lambda case, ops: delta_replicate_corner(ops["x"], ops["w"]),
    "splitk_slice_missing": delta_split_slice,
}
# bug -> the case it is demonstrated on (tests/test_contraction_exact_cpu.py: every bug changes at least one output element of its case)
BUGS = {
    "drop_last_k_ragged_m": "lin_bn128_k448_m260",
    "double_ktile": "lin_ring_bn128_k512_m260",
    "double_k_element": "lin_k4608_ring",
    "halo_wraps_at_right_border": "halo_bn64_ragged",
    "replicate_pad_corner": "halo_bn64_ragged",
    "bias_twice": "lin_ring_bn64_gate_res_inplace",
    "res_row_plus1": "lin_bn64_k96_m127_res_bf16",
    "res_mod_ignored": "lin_swin_180_in_192_res_mod",
    "gate_shift4": "lin_ring_bn64_gate_res_inplace",
    "out2_before_res": "lin_swin_180_in_192_res_mod",
    "vt_head_tail": "pp_none_bf16_vt",
    "splitk_slice_missing": "lin_split3_k1536",
    "idle_block_rewrites_tile0": "lin_xcd_idle_mt65",
}


def plant_vt(case, ref, mask):
    """V^T copy whose head h ends with head h + 1's last row."""
    vt = case["vt"]
    heads = (case["cout"] - vt["col0"]) // vt["hd"]
    r = ref.clone().reshape(vt["batch"], heads, vt["dv"], vt["ld"])
    r[:, :-1, vt["hd"] - 1] = ref.reshape(vt["batch"], heads, vt["dv"], vt["ld"])[:, 1:, vt["hd"] - 1]
    return r.reshape(ref.shape)


# ------------------------------------------------------------------------------------------------------------------------ case table
def _case(kind, name, route, **kw):
    c = dict(kind=kind, name=name, route=route, seed=0, bias=True, act=ACT_NONE, slope=0.0, gate=False, out_scale=1.0, res=None, res_mod=0, out_f32=1,
             out2=False, in_cs=0, out_cs=0, res_cs=0, out2_cs=0, splitk=False, item_rows=0, route_rows=0, vt=None, plain=False, eighths=False,
             inplace=False, phase=False, row=None)
    c.update(kw)
    return c


def lin(name, m, k, n, route, n_pad=None, **kw):
    return _case("linear", name, route, m=m, k=k, cout=n, cout_pad=n_pad or n, **kw)


def conv(name, n, h, w, cin, cout, route, cout_pad=None, stride=1, pad=1, up=0, **kw):
    return _case("conv", name, route, n=n, h=h, w=w, cin=cin, cout=cout, cout_pad=cout_pad or cout, stride=stride, pad=pad, up=up, **kw)


def G(taps, bn, bk, stages, waves, splits=0, padded=0, idle=0):
    """igemm_kernel<128, bn, .., taps, bk, .., stages> on `waves` waves"""
    return dict(kernel=4, form=0, bn=bn, bk=bk, stages=stages, waves=waves, taps=taps, splits=splits, padded=padded, idle=idle)


def R(kernel, form, bn, taps, padded=0, idle=0, vt=0):
    return dict(kernel=kernel, form=form, bn=bn, bk=0, stages=0, waves=0, taps=taps, splits=0, padded=padded, idle=idle, vt=vt)


LIN_ROW, CONV_ROW, PP_ROW = "linear/igemm_kernel<taps=1>", "conv3x3/igemm_kernel<taps=9>", "linear/gemm_pp_kernel"
HALO_ROW, HALO_PP_ROW, S1_ROW = "conv3x3/conv_halo_kernel", "conv3x3/conv_halo_pp_kernel", "conv3x3/conv_halo_s1_kernel"
KERNEL_ROW = {0: S1_ROW, 1: HALO_PP_ROW, 2: PP_ROW, 3: HALO_ROW}
PP_M = 48 * PP_BM    # 48 row tiles x 4 column tiles of N = 1152: gemm_pp_kernel's 192-workgroup threshold
VT = dict(batch=2, T=PP_M // 2, hd=72, dv=80, ld=PP_M // 2 + 64, col0=576)

CASES = [
    # ---- igemm_kernel, taps 1. FIRST: one k-tile on the plain kernel - the premise "MFMA fp32 accumulation is exact on exact sums" on its own
    lin("lin_one_ktile_plain", 128, 64, 128, G(1, 128, 64, 2, 4), plain=True, bias=False),
    lin("lin_one_ktile", 128, 64, 128, G(1, 128, 64, 2, 4)),
    lin("lin_bn32_k32_m1", 1, 32, 96, G(1, 32, 32, 2, 4)),
    lin("lin_bn64_k96_m127_res_bf16", 127, 96, 192, G(1, 64, 32, 2, 4), res="bf16", out_f32=0, out_scale=0.5),
    lin("lin_bn128_k32_m129", 129, 32, 128, G(1, 128, 32, 2, 4), eighths=True),
    lin("lin_bn128_k448_m260", 260, 448, 128, G(1, 128, 64, 2, 4)),                       # 7 k-tiles: below the ring's 8
    lin("lin_bn64_k448_m260", 260, 448, 192, G(1, 64, 64, 2, 4), out_f32=0),
    lin("lin_bn32_k64_n3", 260, 64, 3, G(1, 32, 64, 2, 4), n_pad=32, res="f32"),           # ragged N, out_cs = 3: the scalar epilogue
    lin("lin_ring_bn128_k512_m260", 260, 512, 128, G(1, 128, 64, 4, 8)),                  # 8 k-tiles: the four-tile ring on 8 waves
    lin("lin_ring_bn64_gate_res_inplace", 260, 512, 192, G(1, 64, 64, 4, 8), gate=True, res="f32", inplace=True),
    lin("lin_ring_bn32_k512", 260, 512, 96, G(1, 32, 64, 4, 4), out_f32=0, out2=True, res="bf16"),
    lin("lin_ring_plain_bn128_k512", 260, 512, 128, G(1, 128, 64, 2, 4), plain=True),     # ir_set_plain_kernels: no ring
    lin("lin_swin_180_in_192_res_mod", 129, 192, 180, G(1, 64, 64, 2, 4), n_pad=192, in_cs=224, out_cs=192, res_cs=192, out2_cs=200, res="f32", res_mod=48,
        out2=True, gate=True, out_scale=2.0),
    lin("lin_k4608_ring", 128, 4608, 128, G(1, 128, 64, 4, 8)),
    lin("lin_relu", 129, 64, 64, G(1, 64, 64, 2, 4), act=ACT_LRELU, slope=0.0, out_f32=0),
    lin("lin_gelu_tanh_bf16", 129, 64, 128, G(1, 128, 64, 2, 4), act=ACT_GELU_TANH, out_f32=0, eighths=True),
    lin("lin_gelu_erf_f32", 129, 32, 64, G(1, 64, 32, 2, 4), act=ACT_GELU_ERF, eighths=True),
    lin("lin_silu_f32", 129, 32, 96, G(1, 32, 32, 2, 4), act=ACT_SILU, eighths=True, res="f32"),
    lin("lin_xcd_idle_mt65", 65 * BM - 5, 64, 128, G(1, 128, 64, 2, 4, padded=1, idle=1)),  # 65 row tiles: XCD-padded order, 7 idle blocks
    lin("lin_xcd_mt8", 8 * BM, 64, 256, G(1, 128, 64, 2, 4, padded=1)),
    lin("lin_ring_256_tiles", 128 * BM, 512, 256, G(1, 128, 64, 4, 8, padded=1)),          # 256 workgroups: the ring's last
    lin("lin_ring_272_tiles", 128 * BM + 1, 512, 256, G(1, 128, 64, 2, 4, padded=1, idle=1)),
    lin("lin_split3_k1536", 64, 1536, 128, G(1, 128, 64, 4, 8, splits=3), splitk=True, res="bf16", out_f32=0, gate=True),
    lin("lin_split15_of_16_k8256", 256, 8256, 1024, G(1, 128, 64, 4, 8, splits=15), splitk=True, item_rows=256),   # 129 k-tiles: "no empty split"
    lin("lin_split_batch_item_rows", 256, 1536, 128, G(1, 128, 64, 4, 8, splits=3), splitk=True, item_rows=64, act=ACT_LRELU, slope=0.0),
    # ---- gemm_pp_kernel (k-tiles of 32): its four instantiations at K = 256 - 8 k-tiles exactly, the shortest reduction it takes, where the
    # prologue (4 tiles), the `kt + 3 < KT` / `kt + 4 < KT` switches and the drain sit closest together - and at 16 / 18 k-tiles; whole and
    # ragged M at the 192-workgroup threshold; one k-tile below the shortest reduction, which must report the generic route
    lin("pp_k256_none_bf16_vt", PP_M, PP_MIN_K, 1152, R(2, 0, PP_BN, 1, 1, 0, vt=1), out_f32=0, vt=VT),
    lin("pp_k256_gelu_tanh", PP_M, PP_MIN_K, 1152, R(2, 1, PP_BN, 1, 1, 0), out_f32=0, act=ACT_GELU_TANH, eighths=True),
    lin("pp_k256_gate_res_f32", PP_M, PP_MIN_K, 1152, R(2, 2, PP_BN, 1, 1, 0), gate=True, res="f32"),
    lin("pp_k256_general_ragged", PP_M - 100, PP_MIN_K, 1152, R(2, 3, PP_BN, 1, 1, 0), out_f32=0, res="bf16", out_scale=0.5, out2=True),
    lin("pp_k224_below_min_k", PP_M, PP_MIN_K - PP_BK, 1152, G(1, 128, 32, 2, 4, padded=1), out_f32=0),   # 7 k-tiles: generic, BK 32
    lin("pp_none_bf16_vt", PP_M, 512, 1152, R(2, 0, PP_BN, 1, 1, 0, vt=1), out_f32=0, vt=VT),
    lin("pp_gelu_tanh_ragged", PP_M - 100, 576, 1152, R(2, 1, PP_BN, 1, 1, 0), out_f32=0, act=ACT_GELU_TANH, eighths=True),
    lin("pp_gate_res_f32_inplace", PP_M, 512, 1152, R(2, 2, PP_BN, 1, 1, 0), gate=True, res="f32", inplace=True),
    lin("pp_general_res_bf16_out2", PP_M - 100, 576, 1152, R(2, 3, PP_BN, 1, 1, 0), out_f32=0, res="bf16", out_scale=0.5, out2=True),
    lin("pp_res_mod_leaves_kind1", PP_M, 512, 1152, R(2, 3, PP_BN, 1, 1, 0), res="f32", res_mod=PP_M // 2),
    lin("pp_one_below_threshold", PP_M - PP_BM, 512, 1152, G(1, 128, 64, 2, 4, padded=1, idle=1), out_f32=0),   # 47 x 4 workgroups: generic
    lin("pp_route_rows_forces_generic", PP_M, 512, 1152, G(1, 128, 64, 2, 4, padded=1), out_f32=0, route_rows=PP_M // 2),
    # ---- igemm_kernel, taps 9: stride 2 (pad 0, 1, 0, 1), the folded upsample, BK 32, ragged N, split-K
    conv("conv_s2_bn32_bk32", 1, 16, 24, 32, 32, G(9, 32, 32, 2, 4), stride=2, pad=0),
    conv("conv_s2_ring_bn128", 2, 16, 18, 64, 128, G(9, 128, 64, 4, 8), stride=2, pad=0, res="bf16", out_f32=0),
    conv("conv_s2_ring_bn64", 1, 18, 16, 64, 64, G(9, 64, 64, 4, 8), stride=2, pad=0),
    conv("conv_ring_bn32_cout3", 1, 20, 28, 64, 3, G(9, 32, 64, 4, 4), cout_pad=32),
    conv("conv_bk32_bn64", 2, 9, 17, 32, 64, G(9, 64, 32, 2, 4), out_f32=0),
    conv("conv_bk32_bn128_cin96", 1, 13, 21, 96, 128, G(9, 128, 32, 2, 4)),
    conv("conv_up_bk32_bn64", 1, 12, 20, 32, 64, G(9, 64, 32, 2, 4, padded=1, idle=0), up=1),    # 960 pixels: 8 row tiles
    conv("conv_s2_plain_bn128", 2, 16, 18, 64, 128, G(9, 128, 64, 2, 4), stride=2, pad=0, plain=True),
    conv("conv_s2_plain_bn64", 1, 18, 16, 64, 64, G(9, 64, 64, 2, 4), stride=2, pad=0, plain=True),
    conv("conv_plain_bn32_cout3", 1, 20, 28, 64, 3, G(9, 32, 64, 2, 4), cout_pad=32, plain=True),
    conv("conv_split3_two_images", 2, 8, 8, 192, 128, G(9, 128, 64, 4, 8, splits=3), splitk=True, res="f32"),
    # ---- conv_halo_kernel: 8 x 16 patches, 64- and 128-channel tiles, folded upsample, phase weights
    conv("halo_bn64_whole", 2, 16, 32, 64, 64, R(3, 0, 64, 9, 1, 0), out_f32=0),
    conv("halo_bn64_ragged", 2, 13, 21, 64, 64, R(3, 0, 64, 9, 1, 0), res="f32"),
    conv("halo_bn128_border1", 1, 9, 17, 64, 128, R(3, 0, 128, 9, 0, 0), act=ACT_LRELU, slope=0.25, out_f32=0, res="bf16"),   # border tiles one pixel wide
    conv("halo_bn64_up", 1, 5, 9, 64, 64, R(3, 1, 64, 9, 0, 0), up=1),
    conv("halo_bn128_up", 2, 8, 8, 64, 128, R(3, 1, 128, 9, 0, 0), up=1, out_f32=0),
    conv("halo_bn64_phase", 2, 8, 16, 64, 64, R(3, 2, 64, 9, 1, 0), up=1, phase=True, out_f32=0),
    conv("halo_bn128_phase_ragged", 1, 9, 17, 64, 128, R(3, 2, 128, 9, 1, 0), up=1, phase=True, out_f32=0),
    conv("halo_plain_cin128", 1, 16, 16, 128, 128, R(3, 0, 128, 9, 0, 0), plain=True),   # what conv_halo_pp_kernel takes runs here under plain kernels
    # ---- conv_halo_pp_kernel: 16 x 16 patches x 128 channels
    conv("halo_pp_whole", 2, 16, 32, 128, 128, R(1, 0, 128, 9, 0, 0), out_f32=0, res="bf16"),
    conv("halo_pp_border1", 1, 17, 33, 128, 256, R(1, 0, 128, 9, 0, 0)),
    conv("halo_pp_up", 2, 9, 8, 128, 128, R(1, 1, 128, 9, 0, 0), up=1, out_f32=0),
    conv("halo_pp_below_s1_threshold", 1, 64, 224, 128, 128, R(1, 0, 128, 9, 1, 0), out_f32=0),   # 28 tiles of 16 x 32: one column of tiles short of conv_halo_s1
    # ---- conv_halo_s1_kernel: 16 x 32 patches, from 32 patch tiles per image
    conv("s1_whole", 1, 64, 256, 128, 128, R(0, 0, 0, 9), out_f32=0),
    conv("s1_ragged_res_two_images", 2, 65, 225, 128, 128, R(0, 0, 0, 9), out_f32=0, res="bf16"),
    conv("s1_up", 1, 32, 128, 128, 128, R(0, 1, 0, 9), up=1, out_f32=0),
    conv("s1_up2x2_phase", 1, 64, 256, 128, 128, R(0, 2, 0, 9), up=1, phase=True, out_f32=0),
]
for _i, _c in enumerate(CASES):
    _c["seed"] = 1000 + _i
    _c["row"] = KERNEL_ROW.get(_c["route"]["kernel"], LIN_ROW if _c["kind"] == "linear" else CONV_ROW)
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def route_key(r):
    return (r["kernel"], r["form"], r["bn"], r["bk"], r["stages"], r["waves"], r["taps"])


def route_universe(lib):
    """Every (kernel, form, bn, bk, stages, waves, taps) ir_op_igemm_route can report for bf16 operands, fast and plain kernels: the library
    evaluates its own rule (ir_igemm_route() in csrc/igemm.hip) over a grid of launches that crosses every threshold the rule reads
    (ir_op_igemm_route_range; no device needed), so an instantiation added to the rule appears here without anybody listing it. Not in the
    query's range, because ir_op_conv_ex never sets what selects them: the 4-wave ring at BN 128 / 64 (only with fused GroupNorm statistics:
    ir_op_conv_groupnorm) and conv_halo_s1_kernel's NORM form (ir_op_conv_norm). conv64 appears only where IR_CONV64 is set."""
    import ctypes as C
    from instarevive_amd._lib import igemm_route_fields
    n = lib.ir_op_igemm_route_range(None, 0)
    assert n > 0, n
    buf = (C.c_longlong * n)()
    assert lib.ir_op_igemm_route_range(buf, n) == n
    return {route_key(igemm_route_fields(int(v))) for v in buf}


# routes no case reaches, by name, with the reason
UNREACHED_ALLOWED = {(5, 0, 0, 0, 0, 0, 9): "conv64: opt-in (IR_CONV64), has its own entry ir_op_conv64 and test_conv64_full_resolution"}


def check_complete(universe, cases=None):
    """Every route of `universe` (route_universe()) outside UNREACHED_ALLOWED is some case's route; split-K with taps 1 and 9, with more than 2 slices; each tile
    order (one block per tile, XCD-padded, XCD-padded with idle blocks) on igemm_kernel; plain kernels on the non-ring forms."""
    cases = CASES if cases is None else cases
    reached = {route_key(c["route"]) for c in cases}
    stray = reached - universe
    assert not stray, f"routes outside the universe: {sorted(stray)}"
    missing = universe - reached - set(UNREACHED_ALLOWED)
    assert not missing, f"routes no case reaches: {sorted(missing)}"
    gen = [c for c in cases if c["route"]["kernel"] == 4]
    for taps in (1, 9):
        assert any(c["route"]["splits"] > 2 and c["route"]["taps"] == taps for c in gen), f"no split-K case with taps {taps}"
    for order in ((0, 0), (1, 0), (1, 1)):
        assert any((c["route"]["padded"], c["route"]["idle"]) == order for c in gen), f"no igemm_kernel case with tile order {order}"
    for taps in (1, 9):
        assert any(c["plain"] and c["route"]["taps"] == taps for c in gen), f"no plain-kernel igemm_kernel case with taps {taps}"
    return reached
