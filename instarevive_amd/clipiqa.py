"""CLIP-IQA of results on the device (ir_clipiqa, csrc/clipiqa.hip): the no-reference metric `clipiqa` of the reference's evaluate_img.py, which
tools/evaluate_clipiqa.py restates as a torch model (pyiqa's default: OpenAI CLIP RN50 at the image's own size, the attention pool without
positional embedding, five antonym prompt pairs). The image tower runs behind the network on the uint8 result that is in device memory anyway,
in exact fp32 (fp32-input MFMA) with an fp64 tail; the text side - ten fixed prompts - is encoded once on the CPU when the model is loaded.

load_model() reads the user's RN50.pt (the pretrained weights do not ship with the project) or an .npz, configure() uploads and binds it
(ir_clipiqa_configure), queue_clipiqa() / fetch_clipiqa() / score_arrays() stand beside lpips.queue_lpips() / fetch_lpips() / lpips_arrays(),
ClipIqaSlot holds the scores of one staging slot's batch like niqe.NiqeSlot.
"""
import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

MIN_EDGE = 32             # below it the tower's last map is empty
WS_CAP = 3 << 29          # bytes: a batch is split into calls whose workspace stays under it (one image is always taken whole)


def _model_module():
    """tools/evaluate_clipiqa.py as a module: the model's shapes, key names and loader are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_clipiqa
    return evaluate_clipiqa


def __getattr__(name):
    if name == "ClipIqaError":
        return _model_module().ClipIqaError
    raise AttributeError(name)


def load_model(path, bpe=None) -> dict:
    """evaluate_clipiqa.load_model: the user's OpenAI RN50.pt (TorchScript archive or plain state dict, upcast to float32) or an .npz with the same
    names and optionally the text rows; the text features are computed on the CPU with the BPE table under `bpe`."""
    return _model_module().load_model(path, bpe)


def scaling_table() -> np.ndarray:
    """[3][256] float32: the network's input for byte v of channel c, as the library makes it (ir_clipiqa_scale_table; needs no GPU)."""
    tab = np.zeros((3, 256), np.float32)
    if L.load_library().ir_clipiqa_scale_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise RuntimeError("ir_clipiqa_scale_table failed")
    return tab


def configure(ctx, model: dict) -> None:
    """Upload the model of load_model() and bind it. Replaces an earlier binding of the context."""
    cfg = model["cfg"]
    for k, v in model["sd"].items():
        if k.startswith("visual.") and not k.endswith("num_batches_tracked") and k != "visual.attnpool.positional_embedding":
            ctx.upload("clipiqa." + k[len("visual."):], v.float().contiguous())
    ctx.upload("clipiqa.text", model["text"].float().contiguous())
    layers = (C.c_int * 4)(*cfg["layers"])
    ctx.check(ctx.lib.ir_clipiqa_configure(ctx.h, layers, cfg["width"], cfg["heads"], cfg["out_dim"], model["text"].shape[0] // 2,
                                           C.c_float(model["logit_scale_exp"])), "ir_clipiqa_configure")
    ctx.__dict__["_clipiqa_cfg"] = dict(cfg)


def configured(ctx) -> bool:
    return ctx.__dict__.get("_clipiqa_cfg") is not None


def ws_bytes(ctx, n: int, h: int, w: int) -> int:
    return int(ctx.lib.ir_workspace_bytes(ctx.h, L.STAGE_CLIPIQA, n, h, w, 0, 0, 0))


def images_per_call(ctx, n: int, h: int, w: int) -> int:
    """How many of n images of h x w one call takes with its workspace under WS_CAP (at least one)."""
    k = n
    while k > 1 and ws_bytes(ctx, k, h, w) > WS_CAP:
        k = (k + 1) // 2
    return k


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's CLIP-IQA scratch, grown on demand and kept apart from its workspace (whose address recorded graphs hold). Growing waits for
    the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_clipiqa_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_clipiqa_ws"] = None
        ws = ctx.__dict__["_clipiqa_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def queue_clipiqa(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None, feat: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_clipiqa on the current stream: the top-left h x w of the n images at device address img ([n][rows][pitch] bytes, RGB8). out: a contiguous
    float64 device tensor of n values - by default the context's own small buffer, whose page-locked twin fetch_clipiqa() fills. feat: None or
    a contiguous float32 device tensor [n][out_dim]. The batch goes out in calls of images_per_call() images; the results do not depend on the
    split."""
    if out is None:
        buf = ctx.__dict__.get("_clipiqa_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_clipiqa_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_clipiqa: out must be a contiguous float64 tensor of n values")
    od = ctx.__dict__["_clipiqa_cfg"]["out_dim"] if configured(ctx) else 0
    if feat is not None and (feat.dtype != torch.float32 or feat.numel() < n * od or not feat.is_contiguous()):
        raise ValueError("queue_clipiqa: feat must be a contiguous float32 tensor of n x out_dim values")
    per = images_per_call(ctx, n, h, w) if ws is None else n
    for i in range(0, n, per):
        k = min(per, n - i)
        buf = ws if ws is not None else workspace(ctx, max(ws_bytes(ctx, k, h, w), 256))
        ctx.check(ctx.lib.ir_clipiqa(ctx.h, ctx.stream(), C.c_void_p(img + i * rows * pitch), rows, pitch, k, h, w, C.c_void_p(out.data_ptr() + 8 * i),
                                     C.c_void_p(feat.data_ptr() + 4 * i * od) if feat is not None else None, L.ptr(buf), buf.numel()), "ir_clipiqa")
    return out


def fetch_clipiqa(ctx, n: int) -> List[float]:
    """The scores of the last queue_clipiqa(out=None) of n images: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_clipiqa_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def score_arrays(ctx, img: np.ndarray) -> float:
    """CLIP-IQA of an HWC uint8 RGB array: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise _model_module().ClipIqaError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if min(h, w) < MIN_EDGE:
        raise _model_module().ClipIqaError(f"CLIP-IQA needs at least {MIN_EDGE} x {MIN_EDGE} pixels; the image is {h} x {w}")
    dev = torch.from_numpy(img).to(ctx.device)
    queue_clipiqa(ctx, dev.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_clipiqa(ctx, 1)[0]


class ClipIqaSlot(Pooled):
    """The scores of one staging slot's batch: a float64 device buffer, one value per row, and its page-locked twin. A row is an image of the batch:
    the predictions first, then - when asked for - the stage-1 images. Images below 32 pixels on an edge are not launched and score NaN."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d = self.h = None
        self.shapes: List[Tuple[int, int]] = []

    def plan(self, finals: Sequence[Tuple[int, int]], copies: int = 1) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        if not configured(self.ctx):
            raise ValueError("clipiqa: the context has no CLIP-IQA model (instarevive_amd.clipiqa.configure)")
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
            if min(h, w) >= MIN_EDGE:
                need = max(need, ws_bytes(self.ctx, images_per_call(self.ctx, n, h, w), h, w))
        workspace(self.ctx, need)

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """ir_clipiqa of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current stream.
        results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            out = self.d[first + i:first + k]
            if min(gh, gw) < MIN_EDGE:
                out.fill_(float("nan"))
                continue
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            queue_clipiqa(self.ctx, img, rows, pitch, k - i, gh, gw, out)

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's scores on the current stream."""
        rows = len(self.shapes)
        if rows:
            self.h[:rows].copy_(self.d[:rows], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(clipiqa,) of rows first .. first + count - 1 after the download has completed; NaN for an image without a score."""
        return [(float(v),) for v in self.h[first:first + count].tolist()]
