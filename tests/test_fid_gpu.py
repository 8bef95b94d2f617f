"""ir_fid_features (csrc/fid.hip) through the C ABI and instarevive_amd/fid.py against the float64 model of tests/support/fid_model.py.

The gates are measured from the host model, never from the kernel: 8 x the largest deviation of the fp32 CPU model from the float64 model over
the cases, as max_c |f - ref| / max_c |ref| per image, for the 2048 features (fid_model.feature_gate()) and per block for the thirteen block
means (fid_model.block_gates()); the resized image has no tolerance. tests/test_fid_cpu.py shows that every known way to get FID wrong lands
outside the feature gate. The figures are printed by the tests and recorded in docs/parity.md."""
import os

import numpy as np
import pytest
import torch

from instarevive_amd import _lib as L
from tests.support import fid_model as FM

pytestmark = pytest.mark.gpu
EF = FM.EF
CANARY, OUT_CANARY = 0xA5, -777.0
DIM, BC, RS = L.FID_DIM, L.FID_BLOCK_CHANNELS, 299 * 299 * 3
_bound = {}
_device = {}


def _ctx():
    from instarevive_amd import fid as G
    from instarevive_amd.models import get_context
    ctx = get_context(torch.device("cuda", 0))
    if not _bound.get("ok"):
        G.configure(ctx, FM.weights())
        _bound["ok"] = True
    return ctx


def _err(ctx):
    msg = ctx.lib.ir_last_error(ctx.h)
    return msg.decode() if msg else ""


def _embed(imgs, rows, pitch, seed):
    """The images in the top-left corner of [n][rows][pitch] buffers whose other bytes are noise."""
    buf = np.random.default_rng(seed).integers(0, 256, (len(imgs), rows, pitch), dtype=np.uint8)
    for i, im in enumerate(imgs):
        buf[i, :im.shape[0], :3 * im.shape[1]] = im.reshape(im.shape[0], -1)
    return buf


def _raw_call(ctx, buf, h, w, mode="clean", blocks=True, resized=True, n=None, rows=None, pitch=None, ws_short=0, ws_shift=0, null=None, tables_shift=0, mode_code=None):
    """One ir_fid_features call with canaries around every output -> (return code, features, block means, resized, untouched)."""
    from instarevive_amd import fid as G
    bn, brows, bpitch = buf.shape
    n, rows, pitch = bn if n is None else n, brows if rows is None else rows, bpitch if pitch is None else pitch
    dimg = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    cnt = max(n, 1)
    feat = torch.full((cnt * DIM + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    blk = torch.full((cnt * BC + 4,), OUT_CANARY, dtype=torch.float64, device="cuda")
    res = torch.full((cnt * RS + 4,), OUT_CANARY, dtype=torch.float32, device="cuda")
    need = ctx.ws_bytes(L.STAGE_FID, cnt, 0, 0)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 4096 + 256,), CANARY, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    tab = torch.from_numpy(np.concatenate([np.zeros(8, np.uint8), G.resize_plan(max(h, 1), max(w, 1), mode)])).cuda()
    args = dict(img=L.ptr(dimg), tables=tab.data_ptr() + 8 + tables_shift, features=L.ptr(feat), ws=ws.data_ptr() + ws_shift)
    if null:
        args[null] = None
    rc = ctx.lib.ir_fid_features(ctx.h, ctx.stream(), args["img"], rows, pitch, n, h, w, G.MODES[mode] if mode_code is None else mode_code, args["tables"], args["features"],
                                 L.ptr(blk) if blocks else None, L.ptr(res) if resized else None, args["ws"], need - ws_short)
    torch.cuda.synchronize()
    f, b, r = feat.cpu().numpy(), blk.cpu().numpy(), res.cpu().numpy()
    behind = bool((ws[need + ws_shift:] == CANARY).all())
    untouched = bool((f == OUT_CANARY).all() and (b == OUT_CANARY).all() and (r == OUT_CANARY).all() and (ws == CANARY).all())
    if rc == 0:
        assert np.all(f[n * DIM:] == OUT_CANARY), "values behind the features were written"
        assert np.all(b[n * BC if blocks else 0:] == OUT_CANARY), "values behind the block means (or means that were not asked for) were written"
        assert np.all(r[n * RS if resized else 0:] == OUT_CANARY), "values behind the resized images (or images that were not asked for) were written"
        assert behind, "bytes behind the stated workspace were written"
    return rc, f[:n * DIM].reshape(-1, DIM).copy(), b[:n * BC].reshape(-1, BC).copy(), r[:n * RS].reshape(-1, 299, 299, 3).copy(), untouched


def _call(imgs, mode="clean", rows=None, pitch=None, seed=1, **kw):
    h, w = imgs[0].shape[:2]
    buf = _embed(imgs, rows or h + 5, pitch or 3 * w + 13, seed)
    ctx = _ctx()
    rc, f, b, r, _ = _raw_call(ctx, buf, h, w, mode, **kw)
    ctx.check(rc, "ir_fid_features")
    return f, b, r


def _device_value(name):
    if name not in _device:
        f, b, r = _call([FM.image(name)], FM.CASES[name][3])
        _device[name] = f[0], b[0], r[0]
    return _device[name]


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64 if x.dtype == np.float64 else np.uint32)


SINGLE = ["299x299", "300x301", "64x48", "512x384", "64x48_legacy", "300x301_legacy"]


@pytest.mark.parametrize("name", SINGLE)
def test_resized_image_has_the_definitions_bits(name):
    """Pillow's bits for `clean`, torch's for `legacy` (tests/test_fid_cpu.py holds the numpy model to both)."""
    mode = FM.CASES[name][3]
    want = EF.resize_clean(FM.image(name)) if mode == "clean" else EF.resize_legacy(FM.image(name))
    got = _device_value(name)[2]
    assert np.array_equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} of {got.size} values differ, by {np.abs(got - want).max():.3e} at most"


@pytest.mark.parametrize("name", SINGLE)
def test_block_means_pass_their_gates(name):
    """Per block, so that a failure names the block (and with it the concat slice) that is wrong."""
    got = FM.block_measure(_device_value(name)[1], FM.reference(name)[1])
    gates = FM.block_gates()
    for k, blk in enumerate(EF.BLOCKS):
        print(f"{name} {blk}: device off by {got[k]:.3e} (gate {gates[k]:.3e})")
    bad = {EF.BLOCKS[k]: float(got[k]) for k in range(len(EF.BLOCKS)) if not got[k] <= gates[k]}
    assert not bad, bad


@pytest.mark.parametrize("name", SINGLE)
def test_features_pass_the_gate(name):
    f, b, _ = _device_value(name)
    off = FM.measure(f, FM.reference(name)[0])
    print(f"{name}: device off by {off:.3e} (host fp32 model {FM.measure(FM.host(name)[0], FM.reference(name)[0]):.3e}, gate {FM.feature_gate():.3e})")
    assert np.all(np.isfinite(f)) and off <= FM.feature_gate()
    assert np.array_equal(_bits(f), _bits(b[FM.OFFSETS[-2]:]))   # the features are the last block's means


def test_batch_position_and_repetition_do_not_change_a_bit():
    """Three different images of 40 x 56 in buffers of 47 rows and a pitch of 191 bytes: per image the bits of its single call - features, block
    means and resized image - the same bits on a second call and in another order, and the same features without the optional outputs."""
    imgs = [FM.image(n) for n in FM.BATCH]
    f, b, r = _call(imgs, rows=47, pitch=191)
    singles = [_call([im], rows=41, pitch=3 * 56, seed=9) for im in imgs]
    for k, out in enumerate((f, b, r)):
        assert np.array_equal(_bits(out), _bits(np.concatenate([s[k] for s in singles])))
    for i, n in enumerate(FM.BATCH):
        assert FM.measure(f[i], FM.reference(n)[0]) <= FM.feature_gate()
        assert np.all(FM.block_measure(b[i], FM.reference(n)[1]) <= FM.block_gates())
        assert np.array_equal(_bits(r[i]), _bits(EF.resize_clean(imgs[i])))
    f2, b2, r2 = _call(imgs, rows=47, pitch=191)
    assert np.array_equal(_bits(f2), _bits(f)) and np.array_equal(_bits(b2), _bits(b)) and np.array_equal(_bits(r2), _bits(r))
    f3, _, _ = _call([imgs[2], imgs[0], imgs[1]], rows=47, pitch=191, seed=3)
    assert np.array_equal(_bits(f3), _bits(f[[2, 0, 1]]))
    f4, b4, r4 = _call(imgs, rows=47, pitch=191, blocks=False, resized=False)
    assert np.array_equal(_bits(f4), _bits(f)) and b4.size == 3 * BC and r4.size == 3 * RS


def test_python_layer_gives_the_abi_values():
    from instarevive_amd import fid as G
    ctx = _ctx()
    assert G.configured(ctx) and G.ws_bytes(2) == ctx.ws_bytes(L.STAGE_FID, 2, 0, 0)
    for name in ("64x48", "64x48_legacy"):
        got = G.fid_arrays(ctx, FM.image(name), FM.CASES[name][3])
        assert got.shape == (1, DIM) and np.array_equal(_bits(got[0]), _bits(_device_value(name)[0]))
    feats = G.features_of(ctx, [FM.image(n) for n in FM.BATCH])
    ref = np.stack([FM.reference(n)[0] for n in FM.BATCH])
    got, want = G.frechet_distance(*G.statistics(feats), *G.statistics(ref[[1, 2, 0]] + 0.01)), G.frechet_distance(*G.statistics(ref), *G.statistics(ref[[1, 2, 0]] + 0.01))
    print(f"fid of the device features {got:.9g}, of the float64 model's {want:.9g}")
    assert abs(got - want) <= 1e-4 * want
    with pytest.raises(G.FidError):
        G.fid_arrays(ctx, np.zeros((1, 5, 3), np.uint8))


@pytest.mark.parametrize("what", ["null img", "null tables", "null features", "null ws", "n 0", "h 1", "w 1", "h above rows", "pitch below 3w", "mode 2",
                                  "short ws", "misaligned ws", "misaligned tables"])
def test_argument_errors_write_nothing(what):
    ctx = _ctx()
    img = FM.image("40x56_a")
    buf = _embed([img], 45, 3 * 56 + 4, 2)
    h, w, kw = 40, 56, {}
    if what.startswith("null "):
        kw["null"] = what.split()[1]
    elif what == "n 0":
        kw["n"] = 0
    elif what == "h 1":
        h = 1
    elif what == "w 1":
        w = 1
    elif what == "h above rows":
        kw["rows"] = 39
    elif what == "pitch below 3w":
        kw["pitch"] = 3 * 56 - 1
    elif what == "short ws":
        kw["ws_short"] = 256
    elif what == "misaligned ws":
        kw["ws_shift"] = 128
    elif what == "misaligned tables":
        kw["tables_shift"] = 4
    elif what == "mode 2":
        kw["mode_code"] = 2
    rc, _, _, _, untouched = _raw_call(ctx, buf, h, w, **kw)
    assert rc == -1 and untouched, (what, rc, untouched)
    assert "ir_fid_features" in _err(ctx)


def test_unconfigured_context_and_bad_tensors_are_refused():
    """A fresh context: -14 before ir_fid_configure; one tensor missing or mis-shaped returns -2 and names it; then the binding works."""
    from instarevive_amd import fid as G
    ctx = L.Context(0)
    buf = _embed([FM.image("40x56_a")], 40, 3 * 56, 2)
    rc, _, _, _, untouched = _raw_call(ctx, buf, 40, 56)
    assert rc == L.FID_NOT_CONFIGURED and untouched and "ir_fid_configure" in _err(ctx)
    w = FM.weights()
    for k, v in w.items():
        if k != "fid.Mixed_6d.branch7x7_2.bn_mean":
            ctx.upload(k, v)
    assert ctx.lib.ir_fid_configure(ctx.h) == -2 and "fid.Mixed_6d.branch7x7_2.bn_mean" in _err(ctx) and "missing" in _err(ctx)
    ctx.upload("fid.Mixed_6d.branch7x7_2.bn_mean", w["fid.Mixed_6d.branch7x7_2.bn_mean"])
    ctx.upload("fid.Mixed_5b.branch5x5_2.w", torch.zeros((64, 48, 3, 3)))
    assert ctx.lib.ir_fid_configure(ctx.h) == -2 and "fid.Mixed_5b.branch5x5_2.w" in _err(ctx)
    rc, _, _, _, untouched = _raw_call(ctx, buf, 40, 56)
    assert rc == L.FID_NOT_CONFIGURED and untouched
    G.configure(ctx, w)
    rc, f, _, _, _ = _raw_call(ctx, buf, 40, 56)
    assert rc == 0 and np.array_equal(_bits(f[0]), _bits(_call([FM.image("40x56_a")], rows=41, pitch=3 * 56, seed=9)[0][0]))


def test_tool_scores_folders_with_the_kernel(tmp_path, capsys):
    """tools/evaluate_fid.py --backend gpu over two folders of three PNGs: the value of frechet_distance() over ir_fid_features of the decoded
    files, to the bit, and --save_stats / --stats give the same line."""
    from PIL import Image
    from instarevive_amd import fid as G
    torch.save(FM.state_dict(), tmp_path / "pt_inception.pth")
    imgs = {"a": [FM.image(n) for n in FM.BATCH], "b": [FM.image(n) for n in ("64x48", "40x56_b", "40x56_a")]}
    for d, group in imgs.items():
        os.makedirs(tmp_path / d)
        for i, im in enumerate(group):
            Image.fromarray(im).save(tmp_path / d / f"{i}.png")
    assert EF.main(["--model", str(tmp_path / "pt_inception.pth"), str(tmp_path / "a"), str(tmp_path / "b"), "--backend", "gpu"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    ctx = _ctx()
    fa, fb = G.features_of(ctx, imgs["a"]), G.features_of(ctx, imgs["b"])
    want = G.frechet_distance(*G.statistics(fa), *G.statistics(fb))
    assert "rank-deficient" in out[0] and out[-1] == f"fid: {want:.5f}" and want > 0
    assert EF.main(["--model", str(tmp_path / "pt_inception.pth"), str(tmp_path / "b"), "--backend", "gpu", "--save_stats", str(tmp_path / "b.npz")]) == 0
    assert EF.main(["--model", str(tmp_path / "pt_inception.pth"), str(tmp_path / "a"), "--backend", "gpu", "--stats", str(tmp_path / "b.npz")]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == out[-1]
