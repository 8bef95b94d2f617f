"""DISTS of results against ground truth on the device (ir_dists, csrc/dists.hip): the perceptual metric papers report next to LPIPS, which
tools/evaluate_pairs.py::DISTS restates as a torch model. The device call runs VGG-16's thirteen convolutions in exact fp32 (fp32-input MFMA)
at the image's own size, with fp64 moments and score; it reads the uint8 result that is in device memory anyway and shares ground truth,
eligibility and report with the PSNR-Y / SSIM-Y scorer (metrics.py).

load_weights() reads the user's files (the pretrained weights do not ship with the project), configure() uploads them and binds them
(ir_dists_configure), queue_dists() / fetch_dists() / dists_arrays() stand beside lpips.queue_lpips() / fetch_lpips() / lpips_arrays().
"""
import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from .lpips import _evaluate_pairs

MIN_EDGE = 16   # a limit of the library (ir_dists refuses below it); the definition itself has none
CHANNELS = L.DISTS_CHANNELS


class DistsError(ValueError):
    pass


def tensor_names() -> List[str]:
    """The names ir_dists_configure binds, in order."""
    return [f"dists.c{k}.{p}" for k in range(1, 14) for p in ("w", "b")] + ["dists.alpha", "dists.beta"]


def load_weights(model, vgg=None) -> Dict[str, torch.Tensor]:
    """The tensors ir_dists_configure binds, from one of three forms: `model` = a state dict (or its file) in the DISTS module's names
    (`stage1.0.weight` .. `stage5.28.bias`, `alpha`, `beta`; the `mean`, `std` and `*.filter` buffers are ignored); `model` = `alpha` / `beta`
    alone (DISTS_weights.pt) with `vgg` = torchvision's vgg16-397923af.pth (`features.N.*`; the classifier is ignored); or `model` = an .npz
    (or a dict) in ir_dists_configure's own names. The same KeyError / ValueError as the host model for a missing key or a shape that is not VGG-16's."""
    if isinstance(model, dict) and "dists.alpha" in model:   # already in ir_dists_configure's names
        missing = [k for k in tensor_names() if k not in model]
        if missing:
            raise KeyError(f"{missing[0]} missing")
        return {k: torch.as_tensor(model[k], dtype=torch.float32).contiguous() for k in tensor_names()}
    if isinstance(model, str) and model.endswith(".npz"):
        with np.load(model) as z:
            missing = [k for k in tensor_names() if k not in z.files]
            if missing:
                raise KeyError(f"{model}: {missing[0]} missing")
            return {k: torch.from_numpy(np.ascontiguousarray(z[k], np.float32)) for k in tensor_names()}
    net = _evaluate_pairs().DISTS(model, vgg, "cpu")
    out, k = {}, 0
    for convs in net.stages:
        for w, b in convs:
            k += 1
            out[f"dists.c{k}.w"] = w.contiguous()
            out[f"dists.c{k}.b"] = b.contiguous()
    out["dists.alpha"] = net.alpha.contiguous()
    out["dists.beta"] = net.beta.contiguous()
    return out


def scaling_table() -> np.ndarray:
    """[3][256] float32: the network's input for byte v of channel c, as the library makes it (ir_dists_scale_table; needs no GPU)."""
    tab = np.zeros((3, 256), np.float32)
    if L.load_library().ir_dists_scale_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise DistsError("ir_dists_scale_table failed")
    return tab


def configure(ctx, model, vgg=None) -> None:
    """Upload the weights and bind them. Replaces an earlier binding of the context."""
    for k, v in load_weights(model, vgg).items():
        ctx.upload(k, v)
    ctx.check(ctx.lib.ir_dists_configure(ctx.h), "ir_dists_configure")
    ctx.__dict__["_dists_ready"] = True


def configured(ctx) -> bool:
    return bool(ctx.__dict__.get("_dists_ready"))


def ws_bytes(n: int, h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_DISTS, n, h, w, 0, 0, 0))


def queue_dists(ctx, a: int, a_rows: int, a_pitch: int, b: int, b_rows: int, b_pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None, moments: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_dists on the current stream: the top-left h x w of the n images at device address a ([n][a_rows][a_pitch] bytes, RGB8) against those at b.
    out: a contiguous float64 device tensor of n values - by default the context's own small buffer, whose page-locked twin fetch_dists() fills.
    ws: the scratch; by default a grow-only buffer of the context kept apart from its workspace (whose address recorded graphs hold).
    moments: a contiguous float64 device tensor [n][1475][5] that receives mx, my, vx, vy, cxy of every channel, or None."""
    if out is None:
        buf = ctx.__dict__.get("_dists_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_dists_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_dists: out must be a contiguous float64 tensor of n values")
    if moments is not None and (moments.dtype != torch.float64 or moments.numel() < n * CHANNELS * 5 or not moments.is_contiguous()):
        raise ValueError("queue_dists: moments must be a contiguous float64 tensor of n x 1475 x 5 values")
    if ws is None:
        ws = workspace(ctx, ws_bytes(n, h, w))
    ctx.check(ctx.lib.ir_dists(ctx.h, ctx.stream(), C.c_void_p(a), a_rows, a_pitch, C.c_void_p(b), b_rows, b_pitch, n, h, w, C.c_void_p(out.data_ptr()),
                               None if moments is None else C.c_void_p(moments.data_ptr()), L.ptr(ws), ws.numel()), "ir_dists")
    return out


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's DISTS scratch, grown on demand. Growing waits for the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_dists_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_dists_ws"] = None
        ws = ctx.__dict__["_dists_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def fetch_dists(ctx, n: int) -> List[float]:
    """The scores of the last queue_dists(out=None) of n pairs: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_dists_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def dists_arrays(ctx, a: np.ndarray, b: np.ndarray) -> float:
    """DISTS of two HWC uint8 RGB arrays of equal size: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise DistsError(f"dists_arrays: two HWC uint8 RGB arrays of equal size are needed, got {a.shape} and {b.shape}")
    h, w = a.shape[:2]
    if min(h, w) < MIN_EDGE:
        raise DistsError(f"DISTS is scored from {MIN_EDGE} x {MIN_EDGE} pixels")
    da, db = torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)
    queue_dists(ctx, da.data_ptr(), h, 3 * w, db.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_dists(ctx, 1)[0]
