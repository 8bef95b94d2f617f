"""TOPIQ-NR of results on the device (ir_topiq, csrc/topiq.hip): the no-reference metric `topiq_nr` that the reference's evaluate_img.py names
next to its live metrics, which tools/evaluate_topiq.py restates as a torch model (pyiqa's CFANet in the topiq_nr configuration: a ResNet-50
trunk at the image's own size, gated local pooling, five small transformers and the coarse-to-fine cross-attention). It runs behind the
network on the uint8 result that is in device memory anyway, in exact fp32 (fp32-input MFMA) with fp64 statistics and an fp64 tail.

load_model() reads the user's weights (an .npz in the project's names or pyiqa's .pth; the pretrained weights do not ship with the project),
configure() uploads and binds them (ir_topiq_configure), queue_topiq() / fetch_topiq() / score_arrays() stand beside musiq.queue_musiq() /
fetch_musiq() / score_arrays(), TopiqSlot holds the scores of one staging slot's batch like musiq.MusiqSlot.
"""
import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

MIN_EDGE = 16             # below it ir_topiq refuses the image
WS_CAP = 3 << 29          # bytes: a batch is split into calls whose workspace stays under it (one image is always taken whole)


def _model_module():
    """tools/evaluate_topiq.py as a module: the model's shapes, key names and loader are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_topiq
    return evaluate_topiq


def __getattr__(name):
    if name == "TopiqError":
        return _model_module().TopiqError
    raise AttributeError(name)


def load_model(path, heads=None) -> dict:
    """evaluate_topiq.load_model: an .npz in the project's names, pyiqa's .pth state dict, or a dict of tensors."""
    return _model_module().load_model(path, heads)


def input_table() -> np.ndarray:
    """[3][256] float32: the network's input for byte v of channel c, as the library makes it (ir_topiq_input_table; needs no GPU)."""
    tab = np.zeros((3, 256), np.float32)
    if L.load_library().ir_topiq_input_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise RuntimeError("ir_topiq_input_table failed")
    return tab


def position_table(model: dict, H: int, W: int) -> np.ndarray:
    """[D][H][W] float32: the position table of an H x W token grid as the host states it - the model's float64 bicubic, which the device
    evaluates operation for operation."""
    return _model_module().position_table(model["sd"]["h_emb"], model["sd"]["w_emb"], H, W).numpy()


def scorable(h: int, w: int) -> bool:
    """Whether ir_topiq takes an h x w image: no side below 16."""
    return h >= MIN_EDGE and w >= MIN_EDGE


def configure(ctx, model: dict) -> None:
    """Upload the model of load_model() and bind it. Replaces an earlier binding of the context."""
    cfg = model["cfg"]
    for k, v in model["sd"].items():
        ctx.upload("topiq." + k, v.float().contiguous())
    depths = (C.c_int * 4)(*cfg["depths"])
    ctx.__dict__["_topiq_cfg"] = None
    ctx.check(ctx.lib.ir_topiq_configure(ctx.h, depths, cfg["width"], cfg["dim"], cfg["heads"], cfg["ffn"]), "ir_topiq_configure")
    ctx.__dict__["_topiq_cfg"] = dict(cfg)


def configured(ctx) -> bool:
    return ctx.__dict__.get("_topiq_cfg") is not None


def ws_bytes(ctx, n: int, h: int, w: int) -> int:
    return int(ctx.lib.ir_workspace_bytes(ctx.h, L.STAGE_TOPIQ, n, h, w, 0, 0, 0))


def images_per_call(ctx, n: int, h: int, w: int) -> int:
    """How many of n images of h x w one call takes with its workspace under WS_CAP (at least one)."""
    k = n
    while k > 1 and not 0 < ws_bytes(ctx, k, h, w) <= WS_CAP:
        k = (k + 1) // 2
    return k


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's TOPIQ scratch, grown on demand and kept apart from its workspace (whose address recorded graphs hold). Growing waits for
    the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_topiq_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_topiq_ws"] = None
        ws = ctx.__dict__["_topiq_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def queue_topiq(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None, feat: Optional[torch.Tensor] = None,
                level_means: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_topiq on the current stream: the top-left h x w of the n images at device address img ([n][rows][pitch] bytes, RGB8). out: a contiguous
    float64 device tensor of n values - by default the context's own small buffer, whose page-locked twin fetch_topiq() fills. feat: None or a
    contiguous float32 device tensor [n][dim]; level_means: None or one of [n][5][dim]. The batch goes out in calls of images_per_call()
    images; the results do not depend on the split."""
    if out is None:
        buf = ctx.__dict__.get("_topiq_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_topiq_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_topiq: out must be a contiguous float64 tensor of n values")
    dim = ctx.__dict__["_topiq_cfg"]["dim"] if configured(ctx) else 0
    if feat is not None and (feat.dtype != torch.float32 or feat.numel() < n * dim or not feat.is_contiguous()):
        raise ValueError("queue_topiq: feat must be a contiguous float32 tensor of n x dim values")
    if level_means is not None and (level_means.dtype != torch.float32 or level_means.numel() < n * 5 * dim or not level_means.is_contiguous()):
        raise ValueError("queue_topiq: level_means must be a contiguous float32 tensor of n x 5 x dim values")
    per = images_per_call(ctx, n, h, w) if ws is None else n
    for i in range(0, n, per):
        k = min(per, n - i)
        buf = ws if ws is not None else workspace(ctx, max(ws_bytes(ctx, k, h, w), 256))
        ctx.check(ctx.lib.ir_topiq(ctx.h, ctx.stream(), C.c_void_p(img + i * rows * pitch), rows, pitch, k, h, w, C.c_void_p(out.data_ptr() + 8 * i),
                                   C.c_void_p(feat.data_ptr() + 4 * i * dim) if feat is not None else None,
                                   C.c_void_p(level_means.data_ptr() + 4 * i * 5 * dim) if level_means is not None else None, L.ptr(buf), buf.numel()), "ir_topiq")
    return out


def fetch_topiq(ctx, n: int) -> List[float]:
    """The scores of the last queue_topiq(out=None) of n images: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_topiq_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def score_arrays(ctx, img: np.ndarray) -> float:
    """TOPIQ-NR of an HWC uint8 RGB array: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise _model_module().TopiqError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if not scorable(h, w):
        raise _model_module().TopiqError(f"TOPIQ needs at least {MIN_EDGE} x {MIN_EDGE} pixels; the image is {h} x {w}")
    dev = torch.from_numpy(img).to(ctx.device)
    queue_topiq(ctx, dev.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_topiq(ctx, 1)[0]


class TopiqSlot(Pooled):
    """The scores of one staging slot's batch: a float64 device buffer, one value per row, and its page-locked twin. A row is an image of the batch:
    the predictions first, then - when asked for - the stage-1 images. Images with a side below 16 are not launched and score NaN."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d = self.h = None
        self.shapes: List[Tuple[int, int]] = []

    def plan(self, finals: Sequence[Tuple[int, int]], copies: int = 1) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        if not configured(self.ctx):
            raise ValueError("topiq: the context has no TOPIQ model (instarevive_amd.topiq.configure)")
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
        """ir_topiq of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current stream.
        results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            out = self.d[first + i:first + k]
            if not scorable(gh, gw):
                out.fill_(float("nan"))
                continue
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            queue_topiq(self.ctx, img, rows, pitch, k - i, gh, gw, out)

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's scores on the current stream."""
        rows = len(self.shapes)
        if rows:
            self.h[:rows].copy_(self.d[:rows], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(topiq_nr,) of rows first .. first + count - 1 after the download has completed; NaN for an image without a score."""
        return [(float(v),) for v in self.h[first:first + count].tolist()]
