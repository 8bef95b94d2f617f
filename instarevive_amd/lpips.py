"""LPIPS (v0.1, net alex) of results against ground truth on the device (ir_lpips, csrc/lpips.hip): the third paired metric of the reference's
evaluate_img.py, which tools/evaluate_pairs.py::LPIPS restates as an fp32 torch model. The device call is exact fp32 (fp32-input MFMA) with
fp64 norms and sums, reads the uint8 result that is in device memory anyway and shares ground truth, eligibility and report with the
PSNR-Y / SSIM-Y scorer (metrics.py).

load_weights() reads the user's files by the rules of evaluate_pairs.LPIPS.__init__ (the pretrained weights do not ship with the project),
configure() uploads them and binds them (ir_lpips_configure), queue_lpips() / fetch_lpips() / lpips_arrays() stand beside
metrics.queue_scores() / fetch_scores() / score_arrays().
"""
import ctypes as C
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L

MIN_EDGE = 31   # the smallest edge at which each of the five stages has a pixel (31 -> 7 -> 3 -> 3 -> 1); the host model raises below it


class LpipsError(ValueError):
    pass


def _evaluate_pairs():
    """tools/evaluate_pairs.py as a module: the model's shapes, key names and loader are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_pairs
    return evaluate_pairs


def load_weights(lin, alexnet=None) -> Dict[str, torch.Tensor]:
    """The tensors ir_lpips_configure binds, from the files (or state dicts) evaluate_pairs.LPIPS takes: torchvision's `features.N.*` in `alexnet`
    plus the `lin{k}.model.1.weight` heads in `lin`, or one full lpips.LPIPS().state_dict() (`net.slice*.N.*` + heads) in `lin` alone. The same
    KeyError / ValueError as the host model for a missing key or a shape that is not AlexNet's."""
    net = _evaluate_pairs().LPIPS(alexnet, lin, "cpu")
    out = {}
    for k, ((w, b), lw) in enumerate(zip(net.convs, net.lins)):
        out[f"lpips.c{k + 1}.w"] = w.contiguous()
        out[f"lpips.c{k + 1}.b"] = b.contiguous()
        out[f"lpips.lin{k + 1}"] = lw.reshape(-1).contiguous()
    return out


def scaling_table() -> np.ndarray:
    """[3][256] float32: the network's input for byte v of channel c, as the library makes it (ir_lpips_scale_table; needs no GPU)."""
    tab = np.zeros((3, 256), np.float32)
    if L.load_library().ir_lpips_scale_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise LpipsError("ir_lpips_scale_table failed")
    return tab


def configure(ctx, lin, alexnet=None) -> None:
    """Upload the weights and bind them. Replaces an earlier binding of the context."""
    for k, v in load_weights(lin, alexnet).items():
        ctx.upload(k, v)
    ctx.check(ctx.lib.ir_lpips_configure(ctx.h), "ir_lpips_configure")
    ctx.__dict__["_lpips_ready"] = True


def configured(ctx) -> bool:
    return bool(ctx.__dict__.get("_lpips_ready"))


def ws_bytes(n: int, h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_LPIPS, n, h, w, 0, 0, 0))


def queue_lpips(ctx, a: int, a_rows: int, a_pitch: int, b: int, b_rows: int, b_pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_lpips on the current stream: the top-left h x w of the n images at device address a ([n][a_rows][a_pitch] bytes, RGB8) against those at b.
    out: a contiguous float64 device tensor of n values - by default the context's own small buffer, whose page-locked twin fetch_lpips() fills.
    ws: the scratch; by default a grow-only buffer of the context kept apart from its workspace (whose address recorded graphs hold)."""
    if out is None:
        buf = ctx.__dict__.get("_lpips_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_lpips_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_lpips: out must be a contiguous float64 tensor of n values")
    if ws is None:
        ws = workspace(ctx, ws_bytes(n, h, w))
    ctx.check(ctx.lib.ir_lpips(ctx.h, ctx.stream(), C.c_void_p(a), a_rows, a_pitch, C.c_void_p(b), b_rows, b_pitch, n, h, w, C.c_void_p(out.data_ptr()),
                               L.ptr(ws), ws.numel()), "ir_lpips")
    return out


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's LPIPS scratch, grown on demand. Growing waits for the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_lpips_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_lpips_ws"] = None
        ws = ctx.__dict__["_lpips_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def fetch_lpips(ctx, n: int) -> List[float]:
    """The distances of the last queue_lpips(out=None) of n pairs: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_lpips_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def lpips_arrays(ctx, a: np.ndarray, b: np.ndarray) -> float:
    """LPIPS of two HWC uint8 RGB arrays of equal size: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise LpipsError(f"lpips_arrays: two HWC uint8 RGB arrays of equal size are needed, got {a.shape} and {b.shape}")
    h, w = a.shape[:2]
    if min(h, w) < MIN_EDGE:
        raise LpipsError(f"LPIPS needs images of at least {MIN_EDGE} x {MIN_EDGE} pixels")
    da, db = torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)
    queue_lpips(ctx, da.data_ptr(), h, 3 * w, db.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_lpips(ctx, 1)[0]
