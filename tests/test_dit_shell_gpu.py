"""Segment-level parity of the PixArt DiT shell around its blocks: ir_op_dit_shell (the production dit_update_timestep() / dit_embed() /
dit_control_blocks() / dit_final() / dit_emit() host code of csrc/api.cpp, which dit_tokens_run() and the stage entry points call) on the
configured full-width models against tests/support/dit_shell_ref.py evaluated in float64 with torch on the GPU, TF32 off. Nothing here reads
the library under test for the reference.

Models (R.base_weights / R.micro_weights): width 1152, 16 heads of 72; 3 base layers + 2 control copies; a one-layer sample_size-128 model for the
micro-conditioning tables. Cases: R.CASES, the smallest sizes at which a route or an edge exists (see the comments there). Gates: R.GATES,
derived in tests/test_dit_shell_ref_cpu.py; every case re-measures its emulation (TABLES: the fp32 yardstick, which must stay under an eighth)
in float64 at its own size and asserts that it stays under half of each gate. Each case also checks: the plain route
(ir_set_plain_kernels(1)) is inside the gates and the fast route's rel-L2 is at most 1.15x the plain route's; a second launch gives the same
bits (TABLES: with another key in between, so that the tables are rebuilt); item 1 of a batch equals that item run alone (CONTROL: with its
prompt alone); the profiler rows of the part; the workspace is exactly ir_op_dit_shell_ws bytes, pre-filled with 0xFF bytes, and one byte less
is refused with -20 before anything is written; canaries behind every output are untouched.

Route of the patch linear (K = 32, res_mod = T): igemm.hip's takes_gemm_pp() needs Cin >= GEMM_PP_MIN_K = 8 x 32 = 256, so NO token count
sends it to the 256 x 288 big-tile kernel; every EMBED case, the 16384-row headline launch included, runs igemm_kernel<taps=1> (128 x 128
tiles), whose periodic residual (`m % res_mod`) is therefore the one under test - asserted through the profiler row.

Measured figures: docs/parity.md, section "DiT shell".
"""
from contextlib import contextmanager
from functools import lru_cache
import time

import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import dit_shell_ref as R

pytestmark = pytest.mark.gpu

FAST_OVER_PLAIN = 1.15
K_IGEMM1, K_LN, K_OTHER, K_CROSS = "linear/igemm_kernel<taps=1>", "layernorm/layernorm_*_kernel", "other/layout+glue", "flash_attn/flash_attn_x72_kernel (DiT cross-attention)"
CANARY, TAIL = -1024.0, 4096   # (exact in bf16)
PART = {"tables": R.TABLES, "embed": R.EMBED, "control": R.CONTROL, "final": R.FINAL}
ACP = R.alpha_cumprod(int(R.TIMESTEP))


@contextmanager
def full_precision():
    """No TF32 / reduced-precision products inside the reference."""
    mm, cd = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    prec = torch.get_float32_matmul_precision()
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = mm, cd
        torch.set_float32_matmul_precision(prec)


@lru_cache(maxsize=None)
def model(kind):
    """(ShellWeights, Transformer2DModel, ControlTransformerHalf | None), uploaded once; the context holds ONE DiT, so `bound` re-binds."""
    W = R.base_weights() if kind == "base" else R.micro_weights()
    return (W,) + R.model(W)


def bound(case):
    """The case's model, bound to the context (with its control branch), the position table of the case's grid uploaded."""
    W, m, ctl = model("micro" if R.CASES[case][:2] == ("tables", "micro") else "base")
    (ctl or m)._ready()
    if R.CASES[case][0] != "tables":
        m.ensure_pos(*R.CASES[case][2:4])
    return W, m


def set_prompts(m, y, bias):
    m.invalidate_prompt()
    m.set_prompt(y.cuda(), (bias == 0).float().cuda())


def geometry(case):
    """(n, latent h, latent w, timestep) of the launch."""
    c = R.CASES[case]
    if c[0] == "tables":
        return 1, c[3], c[4], c[2]
    return c[1], 2 * c[2], 2 * c[3], R.TIMESTEP


def guarded(shape, dtype, fill):
    """(tensor of `shape` holding `fill` (a value or a tensor), the canary tail behind it), one allocation."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + TAIL,), CANARY, dtype=dtype, device="cuda")
    flat[:n] = fill.reshape(-1) if isinstance(fill, torch.Tensor) else fill
    return flat[:n].view(shape), flat[n:]


def same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def launch(m, W, case, dev, geo=None, short=0, what="", bf16_copy=True):
    """ir_op_dit_shell on device inputs: (return code, {gate key: output}). The workspace holds exactly ir_op_dit_shell_ws bytes (less `short`)
    of 0xFF; the canaries behind the outputs are checked here, and that a refused call left the outputs as they were."""
    ctx, part = m.ctx, R.CASES[case][0]
    n, h, w, t = geo or geometry(case)
    T, C = n * (h // 2) * (w // 2), W.C
    need = int(ctx.lib.ir_op_dit_shell_ws(ctx.h, PART[part], n, h, w))
    assert need > 0, what
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    nan, f32 = float("nan"), torch.float32
    if part == "tables":
        g = [guarded(s, f32, nan) for s in ((C,), (W.L, 6, C), (max(W.ncopy, 1), 6, C), (2, C))]
        args = (None, None, L.ptr(g[0][0]), L.ptr(g[1][0]), L.ptr(g[2][0]) if W.ncopy else None, L.ptr(g[3][0]))
        outs = {"tables_emb": g[0][0], "tables_modtab": g[1][0], "tables_fmod": g[3][0], **({"tables_ctrl_modtab": g[2][0]} if W.ncopy else {})}
    elif part == "embed":
        g = [guarded((T, C), f32, nan), guarded((T, C), torch.bfloat16, nan)]
        args = (L.ptr(dev[0]), None, L.ptr(g[0][0]), L.ptr(g[1][0]) if bf16_copy else None, None, None)
        outs = {"embed_x": g[0][0], **({"embed_xb": g[1][0]} if bf16_copy else {})}
    elif part == "control":
        g = [guarded((T, C), f32, dev[0]), guarded((T, C), f32, dev[1]), guarded((T, C), torch.bfloat16, dev[1].to(torch.bfloat16))]
        args = (None, None, L.ptr(g[0][0]), L.ptr(g[1][0]), L.ptr(g[2][0]), None)
        outs = {"control": g[0][0], "cs": g[1][0], "csb": g[2][0]}
    else:
        x0 = len(dev) > 1
        g = [guarded((n, 4 if x0 else 8, h, w), f32, nan)]
        args = (L.ptr(dev[0]), L.ptr(dev[1]) if x0 else None, L.ptr(g[0][0]), None, None, None)
        outs = {"x0" if x0 else "final": g[0][0]}
    before = {k: o.clone() for k, o in outs.items()}
    rc = ctx.lib.ir_op_dit_shell(ctx.h, ctx.stream(), PART[part], *args, n, h, w, float(t), ACP, L.ptr(ws), need - short)
    torch.cuda.synchronize()
    for _, tail in g:
        assert bool((tail == CANARY).all()), f"{what}: wrote behind an output"
    if rc != 0:
        for k, o in outs.items():
            assert same(o, before[k]), f"{what}: a refused call (rc {rc}) wrote to {k}"
    if part == "control":
        outs = {"control": outs["control"], "control_upd": outs["control"].double() - dev[0].double()}
    return rc, outs


def run(m, W, case, dev, what, **kw):
    rc, outs = launch(m, W, case, dev, what=what, **kw)
    m.ctx.check(rc, what)
    for k, o in outs.items():
        assert torch.isfinite(o).all(), f"{what}: an element of {k} was not written (or is not finite)"
    return outs


def other_key(case):
    """Another cache key (t, h, w) for a TABLES case: another timestep on the base model; on the micro model the SAME timestep and another size."""
    n, h, w, t = geometry(case)
    if R.CASES[case][1] == "base":
        return n, h, w, t + 7.0
    return (n, w, h, t) if h != w else (n, h + 16, w, t)


def expected(case, plain, W):
    """Profiler launches of one part: {kernel row: count} and {class: count}."""
    part = R.CASES[case][0]
    if part == "tables":      # the table launches are not profiled (as on the stage)
        return {}, {}
    if part == "embed":       # patchify; the patch linear on the 128 x 128-tile kernel at every size (see the module docstring)
        return {K_OTHER: 1, K_IGEMM1: 1}, {"other": 1, "linear": 1}
    if part == "final":       # LayerNorm, the C -> 32 linear, unpatchify / eps_to_x0
        return {K_LN: 1, K_IGEMM1: 1, K_OTHER: 1}, {"layernorm": 1, "linear": 1, "other": 1}
    n, gh, gw = R.CASES[case][1:4]
    blocks, T = W.L + W.ncopy, gh * gw
    pad_init = 1 if (T % 64 == 0 and T >= 256 and not plain) else 0
    # per block: 2 LayerNorms, 6 linears, self- and cross-attention, one V transpose; before_proj and one after_proj per copy; vt_pad_init
    return {K_LN: 2 * blocks, K_CROSS: blocks}, {"layernorm": 2 * blocks, "linear": 6 * blocks + 1 + W.ncopy, "flash_attn": 2 * blocks,
                                                  "transpose": blocks + pad_init}


def profiled(m, W, case, dev, what, plain):
    ctx = m.ctx
    ctx.profile_begin()
    out = run(m, W, case, dev, what)
    rows = {k: v["launches"] for k, v in ctx.profile_end_kernels().items()}
    print(f"ROWS {what}: " + (", ".join(f"{k} x{v}" for k, v in sorted(rows.items())) or "none"))
    want_rows, want_classes = expected(case, plain, W)
    classes = {}
    for k, v in rows.items():
        classes[k.split("/")[0]] = classes.get(k.split("/")[0], 0) + v
    for k, v in want_rows.items():
        assert rows.get(k, 0) == v, f"{what}: {k} launched {rows.get(k, 0)} times, expected {v}"
    assert classes == want_classes, f"{what}: launches per class {classes}, expected {want_classes}"
    return out


def gate(case, what, e, problems, share=1.0):
    """Prints every figure with its share of the gate and notes those outside in `problems` (the case asserts at its end, so that one run shows
    every figure); -> the largest rel-L2."""
    g = R.gates_of(case)
    for key, ek in e.items():
        print(f"MEASURED {what} {key}: rel-L2 {ek[0]:.2e} ({ek[0] / g[key][0]:.2f} of gate)  worst {ek[1]:.2e} ({ek[1] / g[key][1]:.2f} of gate)")
        for v, gv, name in zip(ek, g[key], ("rel-L2", "worst")):
            if not v <= gv * share:
                problems.append(f"{what} {key}: {name} {v:.3e} exceeds {share:g} x its gate {gv:.0e}")
    return max(ek[0] for ek in e.values())


@pytest.mark.parametrize("case", list(R.CASES))
def test_dit_shell(case):
    part = R.CASES[case][0]
    t_start = time.time()
    W, m = bound(case)
    ctx = m.ctx
    what = f"dit shell {case}"
    n, h, w, t = geometry(case)
    cpu = R.case_inputs(case)
    dev = [x.cuda().contiguous() for x in cpu]
    ins64 = tuple(x.double() for x in dev)
    if part == "control":
        set_prompts(m, *R.case_prompts(case))
    with full_precision(), torch.no_grad():
        if part == "tables":
            ref = R.run_case(case, (torch.zeros(1, device="cuda", dtype=torch.float64),))
            emu = R.run_case(case, (torch.zeros(1, device="cuda"),), dtype=torch.float32)
        else:
            ref = R.run_case(case, ins64)
            emu = R.run_case(case, ins64, emulate=True)
        torch.cuda.synchronize()
    t_ref = time.time() - t_start
    problems = []
    gate(case, what + " EMULATION", R.measure(emu, ref), problems, share=1 / R.TABLES_MARGIN if part == "tables" else 0.5)
    del emu

    if part == "tables":   # another key in between: every launch of the case rebuilds the tables, and they follow the key
        o = run(m, W, case, dev, what + " other key", geo=other_key(case))
    a = run(m, W, case, dev, what)
    if part == "tables":
        assert not same(a["tables_emb"], o["tables_emb"]), f"{what}: the tables did not follow the key {other_key(case)[1:]} -> {(h, w, t)}"
        run(m, W, case, dev, what + " other key", geo=other_key(case))
    b = profiled(m, W, case, dev, what + " again", False)
    assert all(same(a[k], b[k]) for k in a), f"{what}: two launches differ"
    l2_fast = gate(case, what, R.measure(a, ref), problems)

    rc, _ = launch(m, W, case, dev, short=1, what=what + " workspace one byte short")
    assert rc == -20, rc

    if part == "embed":    # without the bf16 copy: the same x
        solo = run(m, W, case, dev, what + " without the bf16 copy", bf16_copy=False)
        assert same(solo["embed_x"], a["embed_x"]), f"{what}: x differs when the bf16 copy is not asked for"
    if n > 1:   # item 1 alone (CONTROL: with its prompt alone)
        T1 = (h // 2) * (w // 2)
        one = [x[1:2].contiguous() if x.dim() == 4 else x[T1:2 * T1].contiguous() for x in dev]
        if part == "control" and R.CASES[case][4] > 1:
            y, bias = R.case_prompts(case)
            set_prompts(m, y[1:2], bias[1:2])
        solo = run(m, W, case, one, what + " item 1 alone", geo=(1, h, w, t))
        for k in ("embed_x", "embed_xb", "control", "final", "x0"):
            if k in a:
                a1 = a[k][1:2] if a[k].dim() == 4 else a[k][T1:2 * T1]
                assert same(a1.contiguous(), solo[k]), f"{what}: item 1 of the batch differs from item 1 run alone ({k})"
        if part == "control":
            set_prompts(m, *R.case_prompts(case))

    try:   # the same part on the plain kernels
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        if part == "tables":
            run(m, W, case, dev, what + " other key", geo=other_key(case))
        c = profiled(m, W, case, dev, what + " plain", True)
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
    l2_plain = gate(case, what + " plain", R.measure(c, ref), problems)
    print(f"RATIO {what}: fast / plain rel-L2 {l2_fast / l2_plain:.3f}; reference + emulation {t_ref:.1f} s, case wall time {time.time() - t_start:.1f} s")
    assert not problems, "; ".join(problems)
    assert l2_fast <= FAST_OVER_PLAIN * l2_plain, f"{what}: fast route rel-L2 {l2_fast:.3e} against the plain route's {l2_plain:.3e}"
    del ref, ins64, dev, a, b, c
    torch.cuda.empty_cache()


def test_base_model_after_a_micro_model_has_no_size_terms():
    """ir_dit_configure of a model without micro-conditioning on a context that held a sample_size-128 model: the size embeddings are gone
    from emb (and so from every table), at the timestep the micro model's tables were last built for."""
    Wm, mm, _ = model("micro")
    mm._upload()
    micro = run(mm, Wm, "micro_48x80", [], "micro tables")
    W, m, ctl = model("base")
    m._upload()
    ctl._upload()
    case = "t400"
    with full_precision(), torch.no_grad():
        ref = R.run_case(case, (torch.zeros(1, device="cuda", dtype=torch.float64),))
    got = run(m, W, case, [], "base tables after the micro model")
    problems = []
    gate(case, "base tables after the micro model", R.measure(got, ref), problems)
    assert not problems, "; ".join(problems)
    assert not same(got["tables_emb"], micro["tables_emb"])


def test_dit_shell_refuses_bad_arguments():
    """-1 for a bad part, a missing tensor or an alpha_cumprod outside (0, 1); -10 for a size that is not positive and even; -11 on a context
    without a DiT, for CONTROL without a control branch or without a prompt, for EMBED without the grid's position table; -12 for a prompt count
    that is neither 1 nor n; -20 for a workspace that is too small. Nothing is written then."""
    W, m = bound("control_16x16")
    ctx = m.ctx
    set_prompts(m, *R.case_prompts("control_12x20x2"))   # two prompt slots
    C, T = W.C, 64
    lat = torch.zeros(2, 4, 16, 16, device="cuda")
    ws = torch.full((1 << 26,), 255, dtype=torch.uint8, device="cuda")
    outs = [torch.full((2 * T * 6 * C,), CANARY, device="cuda") for _ in range(4)]
    m.ensure_pos(8, 8)

    def rc(part, in0=lat, in1=None, o=(0, 1, 2, 3), n=2, h=16, w=16, acp=ACP, ws_bytes=ws.numel(), c=ctx):
        for t in outs:
            t.fill_(CANARY)
        p = [L.ptr(outs[i]) if i in o else None for i in range(4)]
        r = c.lib.ir_op_dit_shell(c.h, c.stream(), part, L.ptr(in0), L.ptr(in1), *p, n, h, w, 400.0, acp, L.ptr(ws), ws_bytes)
        torch.cuda.synchronize()
        assert r == 0 or all(bool((t == CANARY).all()) for t in outs), "a refused call wrote to an output"
        return r

    assert rc(R.TABLES) == 0 and rc(R.EMBED) == 0 and rc(R.CONTROL) == 0 and rc(R.FINAL, in0=outs[3], o=(0,)) == 0
    assert rc(R.FINAL, in0=outs[3], in1=lat, o=(0,)) == 0
    assert rc(4) == -1 and rc(-1) == -1
    assert rc(R.TABLES, o=(0, 1, 3)) == -1 and rc(R.TABLES, o=(1, 2, 3)) == -1 and rc(R.EMBED, in0=None) == -1 and rc(R.EMBED, o=()) == -1
    assert rc(R.CONTROL, o=(0, 1)) == -1 and rc(R.FINAL, in0=None) == -1 and rc(R.FINAL, o=()) == -1
    assert rc(R.FINAL, in0=outs[3], in1=lat, o=(0,), acp=0.0) == -1 and rc(R.FINAL, in0=outs[3], in1=lat, o=(0,), acp=1.0) == -1
    for part in (R.TABLES, R.EMBED, R.CONTROL, R.FINAL):
        assert rc(part, h=15) == -10 and rc(part, w=0) == -10 and rc(part, n=0) == -10, part
        assert ctx.lib.ir_op_dit_shell_ws(ctx.h, part, 2, 15, 16) == 0
        assert rc(part, in0=outs[3] if part == R.FINAL else lat, ws_bytes=1024) == -20, part
    assert ctx.lib.ir_op_dit_shell_ws(ctx.h, 4, 2, 16, 16) == 0
    assert rc(R.EMBED, h=18, w=14) == -11                # no dit.pos.9x7
    assert rc(R.CONTROL, n=3) == -12 and rc(R.CONTROL, n=1) == -12
    ctl = model("base")[2]
    ctl._upload()                                          # re-binding the control branch drops the prompt caches
    assert rc(R.CONTROL) == -11
    Wm, mm, _ = model("micro")
    mm._upload()                                           # a model without a control branch
    set_prompts(mm, *R.case_prompts("control_16x16"))
    assert rc(R.CONTROL, n=1) == -11 and ctx.lib.ir_op_dit_shell_ws(ctx.h, R.CONTROL, 1, 16, 16) == 0
    assert rc(R.TABLES, o=(0, 1, 3)) == 0                  # (no ctrl_modtab to ask for)
    bare = L.Context(0)
    for part in (R.TABLES, R.EMBED, R.CONTROL, R.FINAL):
        assert rc(part, c=bare) == -11 and bare.lib.ir_op_dit_shell_ws(bare.h, part, 1, 16, 16) == 0
