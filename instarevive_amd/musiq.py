"""MUSIQ of results on the device (ir_musiq, csrc/musiq.hip): the no-reference metric `musiq` of the reference's evaluate_img.py, which
tools/evaluate_musiq.py restates as a torch model (pyiqa's default koniq10k configuration: three scales, 32 x 32 patches, a ResNet stem per
patch, hashed spatial and scale embeddings, 14 transformer blocks). It runs behind the network on the uint8 result that is in device memory
anyway, in exact fp32 (fp32-input MFMA) with fp64 statistics.

load_model() reads the user's weights (an .npz in the project's names or pyiqa's .pth; the pretrained weights do not ship with the project),
configure() uploads and binds them (ir_musiq_configure; the conv weights go up standardised, as the model reads them), queue_musiq() /
fetch_musiq() / score_arrays() stand beside clipiqa.queue_clipiqa() / fetch_clipiqa() / score_arrays(), MusiqSlot holds the scores of one
staging slot's batch like clipiqa.ClipIqaSlot.
"""
import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

WS_CAP = 3 << 29          # bytes: a batch is split into calls whose workspace stays under it (one image is always taken whole)


def _model_module():
    """tools/evaluate_musiq.py as a module: the model's shapes, key names and loader are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_musiq
    return evaluate_musiq


def __getattr__(name):
    if name == "MusiqError":
        return _model_module().MusiqError
    raise AttributeError(name)


def load_model(path) -> dict:
    """evaluate_musiq.load_model: an .npz in the project's names, pyiqa's .pth state dict, or a dict of tensors."""
    return _model_module().load_model(path)


def input_table() -> np.ndarray:
    """[256] float32: the network's input for byte v, as the library makes it (ir_musiq_input_table; needs no GPU)."""
    tab = np.zeros((256,), np.float32)
    if L.load_library().ir_musiq_input_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise RuntimeError("ir_musiq_input_table failed")
    return tab


def layout(h: int, w: int, longer: Sequence[int] = L.MUSIQ_LONGER, patch: int = 32, grid: int = 10):
    """ir_musiq_layout (needs no GPU): (T, per scale (rh, rw, count_h, count_w, pad_top, pad_left), the hashed index of every patch token), or
    None for a size the library refuses."""
    lib = L.load_library()
    k = len(longer)
    lon = (C.c_int * k)(*longer)
    per = np.zeros((k, 6), np.int32)
    T = lib.ir_musiq_layout(h, w, patch, grid, k, lon, C.c_void_p(per.ctypes.data), None, 0)
    if T < 1:
        return None
    idx = np.zeros((T - 1,), np.int32)
    if lib.ir_musiq_layout(h, w, patch, grid, k, lon, None, C.c_void_p(idx.ctypes.data), T - 1) != T:
        raise RuntimeError("ir_musiq_layout failed")
    return T, [tuple(int(v) for v in row) for row in per], idx


def scorable(h: int, w: int, longer: Sequence[int] = L.MUSIQ_LONGER) -> bool:
    """Whether ir_musiq takes an h x w image: no resized side rounds to 0."""
    k = len(longer)
    return h >= 1 and w >= 1 and L.load_library().ir_musiq_layout(h, w, 32, 10, k, (C.c_int * k)(*longer), None, None, 0) > 0


def configure(ctx, model: dict) -> None:
    """Upload the model of load_model() and bind it. Replaces an earlier binding of the context."""
    cfg = model["cfg"]
    for k, v in model["sd"].items():
        conv = k[:-len(".weight")] if k.endswith(".weight") else None
        ctx.upload("musiq." + k, (model["std"][conv] if conv in model["std"] else v).float().contiguous())
    longer = (C.c_int * len(cfg["longer"]))(*cfg["longer"])
    ctx.check(ctx.lib.ir_musiq_configure(ctx.h, cfg["patch"], cfg["hidden"], cfg["mlp"], cfg["heads"], cfg["layers"], cfg["grid"], len(cfg["longer"]), longer),
              "ir_musiq_configure")
    ctx.__dict__["_musiq_cfg"] = dict(cfg)


def configured(ctx) -> bool:
    return ctx.__dict__.get("_musiq_cfg") is not None


def ws_bytes(ctx, n: int, h: int, w: int) -> int:
    return int(ctx.lib.ir_workspace_bytes(ctx.h, L.STAGE_MUSIQ, n, h, w, 0, 0, 0))


def images_per_call(ctx, n: int, h: int, w: int) -> int:
    """How many of n images of h x w one call takes with its workspace under WS_CAP (at least one)."""
    k = n
    while k > 1 and not 0 < ws_bytes(ctx, k, h, w) <= WS_CAP:
        k = (k + 1) // 2
    return k


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's MUSIQ scratch, grown on demand and kept apart from its workspace (whose address recorded graphs hold). Growing waits for
    the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_musiq_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_musiq_ws"] = None
        ws = ctx.__dict__["_musiq_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def queue_musiq(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None, feat: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_musiq on the current stream: the top-left h x w of the n images at device address img ([n][rows][pitch] bytes, RGB8). out: a contiguous
    float64 device tensor of n values - by default the context's own small buffer, whose page-locked twin fetch_musiq() fills. feat: None or a
    contiguous float32 device tensor [n][hidden]. The batch goes out in calls of images_per_call() images; the results do not depend on the
    split."""
    if out is None:
        buf = ctx.__dict__.get("_musiq_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_musiq_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_musiq: out must be a contiguous float64 tensor of n values")
    hid = ctx.__dict__["_musiq_cfg"]["hidden"] if configured(ctx) else 0
    if feat is not None and (feat.dtype != torch.float32 or feat.numel() < n * hid or not feat.is_contiguous()):
        raise ValueError("queue_musiq: feat must be a contiguous float32 tensor of n x hidden values")
    per = images_per_call(ctx, n, h, w) if ws is None else n
    for i in range(0, n, per):
        k = min(per, n - i)
        buf = ws if ws is not None else workspace(ctx, max(ws_bytes(ctx, k, h, w), 256))
        ctx.check(ctx.lib.ir_musiq(ctx.h, ctx.stream(), C.c_void_p(img + i * rows * pitch), rows, pitch, k, h, w, C.c_void_p(out.data_ptr() + 8 * i),
                                   C.c_void_p(feat.data_ptr() + 4 * i * hid) if feat is not None else None, L.ptr(buf), buf.numel()), "ir_musiq")
    return out


def fetch_musiq(ctx, n: int) -> List[float]:
    """The scores of the last queue_musiq(out=None) of n images: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_musiq_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def score_arrays(ctx, img: np.ndarray) -> float:
    """MUSIQ of an HWC uint8 RGB array: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise _model_module().MusiqError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if not scorable(h, w):
        raise _model_module().MusiqError(f"a resized side of a {h} x {w} image rounds to 0")
    dev = torch.from_numpy(img).to(ctx.device)
    queue_musiq(ctx, dev.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_musiq(ctx, 1)[0]


class MusiqSlot(Pooled):
    """The scores of one staging slot's batch: a float64 device buffer, one value per row, and its page-locked twin. A row is an image of the batch:
    the predictions first, then - when asked for - the stage-1 images. Images of which a resized side rounds to 0 are not launched and score NaN."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d = self.h = None
        self.shapes: List[Tuple[int, int]] = []

    def plan(self, finals: Sequence[Tuple[int, int]], copies: int = 1) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        if not configured(self.ctx):
            raise ValueError("musiq: the context has no MUSIQ model (instarevive_amd.musiq.configure)")
        self.shapes = [tuple(int(v) for v in f) for f in finals] * copies
        rows = len(self.shapes)
        if self.d is None or self.d.numel() < rows:
            cap = max(rows, 16)
            self.d = torch.zeros((cap,), dtype=torch.float64, device=self.ctx.device)
            self.h = torch.zeros((cap,), dtype=torch.float64).pin_memory()

    def reserve(self) -> None:
        """Grow the scratch to what the largest call of this batch needs, before anything of the batch is queued."""
        need = 256
        n = len(self.shapes)
        for h, w in set(self.shapes):
            if scorable(h, w):
                need = max(need, ws_bytes(self.ctx, images_per_call(self.ctx, n, h, w), h, w))
        workspace(self.ctx, need)

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """ir_musiq of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current stream.
        results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            out = self.d[first + i:first + k]
            if not scorable(gh, gw):
                out.fill_(float("nan"))
                continue
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            queue_musiq(self.ctx, img, rows, pitch, k - i, gh, gw, out)

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's scores on the current stream."""
        rows = len(self.shapes)
        if rows:
            self.h[:rows].copy_(self.d[:rows], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(musiq,) of rows first .. first + count - 1 after the download has completed; NaN for an image without a score."""
        return [(float(v),) for v in self.h[first:first + count].tolist()]
