"""Block-level parity of the two text encoders: ir_op_text_block (the production t5_embed() / t5_attn() / t5_ffn() / t5_final() and clip_*() host code
of csrc/api.cpp, which t5_run() / clip_text_run() chain for ir_t5_encode / ir_clip_text_encode) on seeded models against
tests/support/text_block_ref.py evaluated in float64 with torch on the GPU, TF32 off. Nothing here reads the library under test for the reference.

Models and cases: R.MODELS / R.CASES (see the comments there: the smallest sizes at which an edge of t5_attn_kernel exists - 1 token, one query tile
and one row more, two items of different lengths, 300 tokens (distances >= 128 on valid keys, LDS above 64 KiB), 512 tokens at dk 64 and 32, a hole
in the mask, no mask, a fully masked item, peaky logits, outlier channels - and the full widths of T5 v1.1 XXL and of ViT-H's text tower in one
layer). Gates: R.GATES / R.CASE_GATES, derived in tests/test_text_block_ref_cpu.py; every case re-measures its emulation in float64 at its own size
and asserts that it stays under half of each gate. Each case also checks: the attention kernel's own output against a float64 softmax over the
q|k|v rows it read; the plain route (ir_set_plain_kernels(1)) is inside the gates; a second launch gives the same bits; every item of a batch
equals that item run alone; the profiler's launches per class; the workspace is exactly ir_op_text_block_ws bytes, pre-filled with 0xFF bytes, and
one byte less is refused with -20 before anything is written; canaries behind every output are untouched. The chain cases run every part through
the entry and ask for the bits of ir_t5_encode / ir_clip_text_encode on the same inputs: the entry runs the stage's code.

Measured figures: docs/parity.md, section "Text encoders".
"""
from contextlib import contextmanager
from functools import lru_cache
import time

import pytest
import torch

from instarevive_amd import _lib as L
from instarevive_amd import weights as PW
from tests.support import text_block_ref as R

pytestmark = pytest.mark.gpu

CANARY, TAIL = -1024.0, 4096   # (exact in bf16)
PART = {"embed": L.TEXT_EMBED, "attn": L.TEXT_ATTN, "ffn": L.TEXT_FFN, "final": L.TEXT_FINAL}
ORDER = sorted(R.CASES, key=lambda c: (R.CASES[c][1], list(R.CASES).index(c)))   # grouped by model: a model of the same family is re-bound on a switch


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
def model(name):
    """(TextWeights, the production model), uploaded once; the context holds ONE model per family, so `bound` re-binds."""
    W = R.weights(name)
    return W, R.model(W)


def bound(name, T=None):
    """The model, bound to the context; for T5 with the position-bias table of T tokens uploaded as the production host code builds it."""
    W, m = model(name)
    m._ready()
    if W.which == R.T5 and T is not None and T not in m._bias_lengths:
        m._bias_lengths.add(T)
        m.ctx.upload(f"t5.bias.{T}", PW.t5_position_bias(m._sd[R.REL], T, R.NB, R.MAXD))
    return W, m


def guarded(shape, dtype, fill):
    """(tensor of `shape` holding `fill` (a value or a tensor), the canary tail behind it), one allocation."""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + TAIL,), CANARY, dtype=dtype, device="cuda")
    flat[:n] = fill.reshape(-1) if isinstance(fill, torch.Tensor) else fill
    return flat[:n].view(shape), flat[n:]


def same(a, b):
    v = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(v(a), v(b))


def launch(m, W, part, layer, B, T, ids=None, x=None, mask=None, short=0, what="", extras=True):
    """ir_op_text_block on device inputs: (return code, {name: output}). The workspace holds exactly ir_op_text_block_ws bytes (less `short`) of
    0xFF; the canaries behind the outputs are checked here, and that a refused call left the outputs as they were."""
    ctx = m.ctx
    need = int(ctx.lib.ir_op_text_block_ws(ctx.h, W.which, PART[part], B, T))
    assert need > 0, what
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    BT, HD, nan = B * T, W.H * W.dk, float("nan")
    gx = guarded((BT, W.D), torch.float32, nan if part == "embed" else x)
    g, outs, qkv, att, out = [gx], {"x": gx[0]}, None, None, None
    if part == "attn" and extras:
        gq, ga = guarded((BT, 3 * HD), torch.bfloat16, nan), guarded((BT, HD), torch.bfloat16, nan)
        g += [gq, ga]
        outs.update(qkv=gq[0], att=ga[0])
        qkv, att = gq[0], ga[0]
    if part == "final":
        go = guarded((BT, W.D), torch.float32, nan)
        g.append(go)
        outs["out"] = out = go[0]
    before = {k: o.clone() for k, o in outs.items()}
    rc = ctx.lib.ir_op_text_block(ctx.h, ctx.stream(), W.which, PART[part], layer, L.ptr(ids), L.ptr(mask), L.ptr(gx[0]), L.ptr(qkv), L.ptr(att),
                                  L.ptr(out), B, T, L.ptr(ws), need - short)
    torch.cuda.synchronize()
    for _, tail in g:
        assert bool((tail == CANARY).all()), f"{what}: wrote behind an output"
    if rc != 0 and rc != -32:   # (-32 is found behind the launches, as on the stage: the rows are written, those of a bad id from row 0)
        for k, o in outs.items():
            assert same(o, before[k]), f"{what}: a refused call (rc {rc}) wrote to {k}"
    if part == "final":
        assert same(outs["x"], before["x"]), f"{what}: FINAL wrote to its input"
    return rc, outs


def run(m, W, part, layer, B, T, what, **kw):
    rc, outs = launch(m, W, part, layer, B, T, what=what, **kw)
    m.ctx.check(rc, what)
    for k, o in outs.items():
        assert torch.isfinite(o).all(), f"{what}: an element of {k} was not written (or is not finite)"
    return outs


def expected_classes(W, part):
    """Profiler launches of one part per class."""
    if part == "embed":      # the gather; CLIP: + the position rows
        return {"other": 1 if W.which == R.T5 else 2}
    if part == "final":
        return {"layernorm": 1}
    if part == "attn":       # norm, q|k|v, attention, o-projection
        return {"layernorm": 1, "linear": 2, "other": 1}
    return {"layernorm": 1, "linear": 2, "other": 1} if W.which == R.T5 else {"layernorm": 1, "linear": 2}   # T5: + the gated-GELU product


def profiled(m, W, part, layer, B, T, what, **kw):
    ctx = m.ctx
    ctx.profile_begin()
    out = run(m, W, part, layer, B, T, what, **kw)
    rows = {k: v["launches"] for k, v in ctx.profile_end_kernels().items()}
    print(f"ROWS {what}: " + (", ".join(f"{k} x{v}" for k, v in sorted(rows.items())) or "none"))
    classes = {}
    for k, v in rows.items():
        classes[k.split("/")[0]] = classes.get(k.split("/")[0], 0) + v
    assert classes == expected_classes(W, part), f"{what}: launches per class {classes}, expected {expected_classes(W, part)}"
    return out


def gate(case, what, e, problems, share=1.0):
    """Prints every figure with its share of the gate and notes those outside in `problems` (the case asserts at its end, so that one run shows
    every figure)."""
    g = R.gates_of(case)
    for key, ek in e.items():
        sh = [ek[i] / g[key][i] if g[key][i] > 0 else (0.0 if ek[i] == 0 else float("inf")) for i in (0, 1)]
        print(f"MEASURED {what} {key}: rel-L2 {ek[0]:.2e} ({sh[0]:.2f} of gate)  worst {ek[1]:.2e} ({sh[1]:.2f} of gate)")
        for v, gv, name in zip(ek, g[key], ("rel-L2", "worst")):
            if not v <= gv * share:
                problems.append(f"{what} {key}: {name} {v:.3e} exceeds {share:g} x its gate {gv:.0e}")


def as_case(part, W, o, x_in):
    """The entry's outputs under the reference's keys."""
    if part == "embed":
        return {"embed": o["x"]}
    if part == "final":
        return {"final": o["out"]}
    return {part: o["x"], part + "_upd": o["x"].double() - x_in.double()}


def measured(case, W, part, o, x_in, ref, B, T, mask):
    e = R.measure(case, as_case(part, W, o, x_in), ref)
    if part == "attn" and "qkv" in o:   # the attention kernel alone: a float64 softmax over the bf16 q|k|v rows it read
        a64 = R.att_from_qkv(W, o["qkv"].double(), B, T, mask)
        e[R.prefix(case) + "att"] = R.errors(o["att"], a64)
    return e


def chain_through_entry(m, W, ids, mask, B, T, what, keep=False):
    """EMBED -> (ATTN, FFN) x L -> FINAL through ir_op_text_block; -> the final rows (keep: every part's output, in order)."""
    x = run(m, W, "embed", 0, B, T, what + " embed", ids=ids)["x"]
    parts = [x]
    for l in range(W.L):
        x = run(m, W, "attn", l, B, T, f"{what} attn {l}", x=x, mask=mask, extras=False)["x"]
        parts.append(x)
        x = run(m, W, "ffn", l, B, T, f"{what} ffn {l}", x=x)["x"]
        parts.append(x)
    out = run(m, W, "final", 0, B, T, what + " final", x=x)["out"]
    return parts + [out] if keep else out


def stage(m, W, ids, mask):
    """ir_t5_encode / ir_clip_text_encode on the same inputs: [B * T][D]."""
    if W.which == R.T5:
        out = m(input_ids=ids, attention_mask=mask)["last_hidden_state"]
    else:
        out = m.encode_with_transformer(ids)
    torch.cuda.synchronize()
    return out.reshape(-1, W.D)


@pytest.mark.parametrize("case", ORDER)
def test_text_block(case):
    part, name, layer, B, T, _, _ = R.CASES[case]
    t_start = time.time()
    W, m = bound(name, T)
    ctx = m.ctx
    what = f"text block {case}"
    ids, x, mask = R.case_inputs(case)
    ids_d = None if ids is None else ids.to("cuda", torch.int32).contiguous()
    x_d = None if x is None else x.cuda().contiguous()
    mask_d = None if mask is None else mask.cuda().contiguous()
    ins = (None if ids is None else ids.cuda(), None if x is None else x_d.double(), mask_d)
    with full_precision(), torch.no_grad():
        ref = R.run_case(case, ins)
        emu = R.run_case(case, ins, emulate=True)
        e_emu = R.measure(case, emu, ref)
        if part == "attn":
            a64 = R.att_from_qkv(W, emu["qkv"], B, T, mask_d)
            e_emu[R.prefix(case) + "att"] = R.errors(R.rb(a64), a64)
        torch.cuda.synchronize()
    t_ref = time.time() - t_start
    problems = []
    gate(case, what + " EMULATION", e_emu, problems, share=0.5)
    del emu

    if part == "chain":   # every part through the entry: the bits of the stage, and inside the chain's gate
        got = chain_through_entry(m, W, ids_d, mask_d, B, T, what)
        want = stage(m, W, ids_d, mask_d)
        assert torch.isfinite(want).all(), f"{what}: the stage's output is not finite"
        assert same(got, want), f"{what}: the parts chained through ir_op_text_block differ from the stage entry"
        gate(case, what, R.measure(case, {"chain": got}, ref), problems)
        try:
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
            gate(case, what + " plain", R.measure(case, {"chain": stage(m, W, ids_d, mask_d)}, ref), problems)
        finally:
            ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
        print(f"TIME {what}: reference + emulation {t_ref:.1f} s, case wall time {time.time() - t_start:.1f} s")
        assert not problems, "; ".join(problems)
        return

    kw = dict(ids=ids_d, x=x_d, mask=mask_d if part == "attn" else None)
    a = run(m, W, part, layer, B, T, what, **kw)
    b = profiled(m, W, part, layer, B, T, what + " again", **kw)
    assert all(same(a[k], b[k]) for k in a), f"{what}: two launches differ"
    with full_precision(), torch.no_grad():
        gate(case, what, measured(case, W, part, a, x_d, ref, B, T, mask_d), problems)

    rc, _ = launch(m, W, part, layer, B, T, short=1, what=what + " workspace one byte short", **kw)
    assert rc == -20, rc

    if part == "attn":   # without the optional outputs: the same stream
        solo = run(m, W, part, layer, B, T, what + " without q|k|v and att", extras=False, **kw)
        assert same(solo["x"], a["x"]), f"{what}: x differs when the optional outputs are not asked for"
    if B > 1:   # every item alone
        for i in range(B):
            one = dict(ids=None if ids_d is None else ids_d[i:i + 1].contiguous(), x=None if x_d is None else x_d[i * T:(i + 1) * T].contiguous(),
                       mask=None if kw["mask"] is None else mask_d[i:i + 1].contiguous())
            solo = run(m, W, part, layer, 1, T, f"{what} item {i} alone", **one)
            for k in a:
                assert same(a[k][i * T:(i + 1) * T].contiguous(), solo[k]), f"{what}: item {i} of the batch differs from item {i} run alone ({k})"

    try:   # the same part on the plain kernels
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 1), "ir_set_plain_kernels")
        c = profiled(m, W, part, layer, B, T, what + " plain", **kw)
    finally:
        ctx.check(ctx.lib.ir_set_plain_kernels(ctx.h, 0), "ir_set_plain_kernels")
    with full_precision(), torch.no_grad():
        gate(case, what + " plain", measured(case, W, part, c, x_d, ref, B, T, mask_d), problems)
    print(f"TIME {what}: reference + emulation {t_ref:.1f} s, case wall time {time.time() - t_start:.1f} s")
    assert not problems, "; ".join(problems)


def test_fully_masked_item_attends_uniformly():
    """T = 24, b = 3 with item 1 fully masked through the STAGE entry (ir_t5_encode): every row is finite (the parent commit's kernel gave 0 / 0
    = NaN on item 1), item 1 is inside the chain's gate against the reference's uniform rule, and items 0 and 2 are bit-equal to running them alone."""
    case = "t5_chain_dk32"
    _, name, _, B, T, _, _ = R.CASES[case]
    W, m = bound(name, T)
    ids, _, mask = R.case_inputs(case)
    assert float(mask[1].sum()) == 0
    ids_d, mask_d = ids.to("cuda", torch.int32).contiguous(), mask.cuda().contiguous()
    got = stage(m, W, ids_d, mask_d)
    assert torch.isfinite(got).all(), "a fully masked item gave rows that are not finite"
    with full_precision(), torch.no_grad():
        ref = R.chain(W, ids.cuda(), mask_d)
    e = R.errors(got[T:2 * T], ref[T:2 * T])
    g = R.gates_of(case)["t5_chain"]
    print(f"MEASURED fully masked item: rel-L2 {e[0]:.2e} ({e[0] / g[0]:.2f} of gate)  worst {e[1]:.2e} ({e[1] / g[1]:.2f} of gate)")
    assert e[0] <= g[0] and e[1] <= g[1], e
    for i in (0, 2):
        alone = stage(m, W, ids_d[i:i + 1].contiguous(), mask_d[i:i + 1].contiguous())
        assert same(got[i * T:(i + 1) * T].contiguous(), alone), f"item {i} beside a fully masked item differs from item {i} run alone"


@pytest.mark.parametrize("name,B", [("clip2", 1), ("clip4", 3), ("vith1", 2)])
def test_clip_parts_are_causal(name, B):
    """No tolerance: changing the ids behind position p leaves rows <= p of EVERY part's output bit-identical."""
    W, m = bound(name)
    T = W.T
    ids = R.make_ids(B, T, W.vocab, 31)
    pa = chain_through_entry(m, W, ids.to("cuda", torch.int32), None, B, T, f"causal {name}", keep=True)
    for p in (0, 8, 63, 64, 75):
        other = ids.clone()
        other[:, p + 1:] = (other[:, p + 1:] + 7) % W.vocab
        assert not torch.equal(other, ids)
        pb = chain_through_entry(m, W, other.to("cuda", torch.int32), None, B, T, f"causal {name} changed behind {p}", keep=True)
        assert len(pa) == 2 + 2 * W.L
        for k, (xa, xb) in enumerate(zip(pa, pb)):
            va, vb = xa.view(B, T, W.D), xb.view(B, T, W.D)
            assert same(va[:, :p + 1].contiguous(), vb[:, :p + 1].contiguous()), f"{name}: part {k} of the chain looked behind position {p}"
            assert not same(va[:, p + 1:].contiguous(), vb[:, p + 1:].contiguous())


@pytest.mark.parametrize("name", ["narrow64", "clip4"])
def test_embed_refuses_an_id_outside_the_vocabulary(name):
    """-32 for an id outside [0, vocab), as on the stage; the flag is cleared with the refusal: the next good call succeeds."""
    W, m = bound(name)
    B, T = 2, (40 if W.which == R.T5 else W.T)
    good = R.make_ids(B, T, W.vocab, 41).to("cuda", torch.int32)
    assert int(good.min()) == 0 and int(good.max()) == W.vocab - 1   # the first and the last row of the table are legal
    first = run(m, W, "embed", 0, B, T, "embed", ids=good)
    for bad_id in (W.vocab, -1):
        bad = good.clone()
        bad[1, 3] = bad_id
        rc, _ = launch(m, W, "embed", 0, B, T, ids=bad, what="embed with a bad id")
        assert rc == -32, rc
        assert b"outside" in m.ctx.lib.ir_last_error(m.ctx.h)
        again = run(m, W, "embed", 0, B, T, "embed after a refusal", ids=good)
        assert same(first["x"], again["x"])


def test_text_block_refuses_bad_arguments():
    """-1 for a bad encoder, part or layer, a missing tensor or a missing t5.bias table; -10 for a bad size (CLIP: any length but the configured
    one); -11 on a context without the model; -20 for a workspace that is too small. Nothing is written then."""
    W, m = bound("narrow64", 40)
    Wc, mc = bound("clip2")
    ctx = m.ctx
    assert ctx is mc.ctx
    ws = torch.full((1 << 24,), 255, dtype=torch.uint8, device="cuda")
    x = torch.full((2 * 77 * 256 + 16,), CANARY, device="cuda")
    out = torch.full((2 * 77 * 256 + 16,), CANARY, device="cuda")
    ids = torch.ones(2, 77, dtype=torch.int32, device="cuda")

    def rc(which, part, layer=0, b=2, t=40, ids=ids, x=x, out=out, ws_bytes=ws.numel(), c=ctx):
        for tt in (x, out):
            if tt is not None:
                tt.fill_(CANARY)
        r = c.lib.ir_op_text_block(c.h, c.stream(), which, part, layer, L.ptr(ids), None, L.ptr(x), None, None, L.ptr(out), b, t, L.ptr(ws), ws_bytes)
        torch.cuda.synchronize()
        assert r == 0 or all(tt is None or bool((tt == CANARY).all()) for tt in (x, out)), "a refused call wrote to an output"
        return r

    for part in range(4):
        assert rc(R.T5, part) == 0 and rc(R.CLIP, part, t=77) == 0, part
    assert rc(2, 0) == -1 and rc(-1, 0) == -1 and rc(R.T5, 4) == -1 and rc(R.T5, -1) == -1
    assert rc(R.T5, L.TEXT_ATTN, layer=2) == -1 and rc(R.T5, L.TEXT_FFN, layer=-1) == -1 and rc(R.CLIP, L.TEXT_ATTN, layer=3, t=77) == -1
    assert rc(R.T5, L.TEXT_ATTN, t=41) == -1                       # no t5.bias.41
    assert rc(R.T5, L.TEXT_EMBED, ids=None) == -1 and rc(R.T5, L.TEXT_FINAL, out=None) == -1 and rc(R.T5, L.TEXT_FFN, x=None) == -1
    for which, t in ((R.T5, 40), (R.CLIP, 77)):
        for part in range(4):
            assert rc(which, part, b=0, t=t) == -10 and rc(which, part, t=0) == -10 and rc(which, part, t=513) == -10, (which, part)
            assert ctx.lib.ir_op_text_block_ws(ctx.h, which, part, 2, 0) == 0
            assert rc(which, part, t=t, ws_bytes=1024) == -20, (which, part)
    assert rc(R.CLIP, L.TEXT_FFN, t=76) == -10 and rc(R.CLIP, L.TEXT_EMBED, t=40) == -10
    assert ctx.lib.ir_op_text_block_ws(ctx.h, 2, 0, 2, 40) == 0 and ctx.lib.ir_op_text_block_ws(ctx.h, R.T5, 4, 2, 40) == 0
    bare = L.Context(0)
    for which, t in ((R.T5, 40), (R.CLIP, 77)):
        for part in range(4):
            assert rc(which, part, t=t, c=bare) == -11 and bare.lib.ir_op_text_block_ws(bare.h, which, part, 2, t) == 0
