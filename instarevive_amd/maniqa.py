"""MANIQA of results on the device (ir_maniqa, csrc/maniqa.hip): the no-reference metric `maniqa` of the reference's evaluate_img.py, which
tools/evaluate_maniqa.py restates as a torch model (pyiqa's koniq configuration: 20 crops of 224 x 224, a ViT-B/8 trunk tapped at blocks
6 .. 9, transposed attention over the channels, two Swin stages, a weighted mean of per-patch scores over all crops). It runs behind the
network on the uint8 result that is in device memory anyway, in exact fp32 (fp32-input MFMA) with fp64 statistics.

The crop origins are an INPUT of the device call: crop_origins() makes them on the host - pyiqa's uniform grid (ir_maniqa_crops) or, with
mode="random", draws keyed by a seed and the file's name - and queue_maniqa() checks them before the upload, so the device computes a pure
function of (image, origins, weights).

load_model() reads the user's weights (an .npz in the project's names or pyiqa's .pth; the pretrained weights do not ship with the project),
configure() uploads and binds them (ir_maniqa_configure), queue_maniqa() / fetch_maniqa() / score_arrays() stand beside
musiq.queue_musiq() / fetch_musiq() / score_arrays(), ManiqaSlot holds the scores of one staging slot's batch like musiq.MusiqSlot.
"""
import ctypes as C
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

WS_CAP = 3 << 29          # bytes: a call's crops are processed in passes whose workspace stays under it (one crop is always taken whole)


def _model_module():
    """tools/evaluate_maniqa.py as a module: the model's shapes, key names, loader and the random origins are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_maniqa
    return evaluate_maniqa


def __getattr__(name):
    if name in ("ManiqaError", "DEFAULT_SEED"):
        return getattr(_model_module(), name)
    raise AttributeError(name)


def load_model(path, cfg=None) -> dict:
    """evaluate_maniqa.load_model: an .npz in the project's names, pyiqa's .pth state dict, or a dict of tensors."""
    return _model_module().load_model(path, cfg)


def input_table() -> np.ndarray:
    """[256] float32: the network's input for byte v, as the library makes it (ir_maniqa_input_table; needs no GPU)."""
    tab = np.zeros((256,), np.float32)
    if L.load_library().ir_maniqa_input_table(C.c_void_p(tab.ctypes.data)) != 0:
        raise RuntimeError("ir_maniqa_input_table failed")
    return tab


def scorable(h: int, w: int, crop: int = 224) -> bool:
    """Whether ir_maniqa takes an h x w image: its short side is above the crop."""
    return min(h, w) > crop


def crop_origins(h: int, w: int, crop: int, crops: int, mode: str = "uniform", seed=None, name=None) -> List[Tuple[int, int]]:
    """[(y, x)] * crops: the uniform grid from the library (ir_maniqa_crops; needs no GPU), or evaluate_maniqa's random draws keyed by `seed`
    and the file's name. ManiqaError for an image whose short side is not above the crop."""
    EM = _model_module()
    if mode != "uniform":
        return EM.crop_origins(h, w, crop, crops, mode, seed, name)
    out = np.zeros((max(crops, 1), 2), np.int32)
    if L.load_library().ir_maniqa_crops(h, w, crop, crops, C.c_void_p(out.ctypes.data)) != 0:
        raise EM.ManiqaError(f"a {h} x {w} image has no {crops} crops of {crop} x {crop} (the short side must be above {crop})")
    return [(int(y), int(x)) for y, x in out[:crops]]


def configure(ctx, model: dict, mode: str = "uniform", seed=None) -> None:
    """Upload the model of load_model() and bind it. Replaces an earlier binding of the context. mode / seed: how ManiqaSlot and score_arrays()
    place the crops when no origins are given."""
    cfg = model["cfg"]
    for k, v in model["sd"].items():
        ctx.upload("maniqa." + k, v.float().contiguous())
    taps = (C.c_int * 4)(*cfg["taps"])
    ctx.check(ctx.lib.ir_maniqa_configure(ctx.h, cfg["crop"], cfg["patch"], cfg["embed"], cfg["vit_heads"], cfg["vit_mlp"], cfg["vit_layers"], taps, cfg["window"],
                                          cfg["swin_heads"], cfg["swin_depth"], cfg["dim_mlp"], C.c_float(cfg["scale"])), "ir_maniqa_configure")
    ctx.__dict__["_maniqa_cfg"] = dict(cfg, mode=mode, seed=seed)


def configured(ctx) -> bool:
    return ctx.__dict__.get("_maniqa_cfg") is not None


def ws_bytes(ctx, n: int, crops: int, per_pass: int = 0) -> int:
    """The workspace of a call of n images with `crops` crops each that takes per_pass crops in a pass (0: one, the least)."""
    return int(ctx.lib.ir_workspace_bytes(ctx.h, L.STAGE_MANIQA, n, 0, 0, crops, per_pass, 0))


def crops_per_pass(ctx, n: int, crops: int) -> int:
    """How many of the n * crops crops one pass takes with the workspace under WS_CAP (at least one)."""
    k = n * crops
    while k > 1 and not 0 < ws_bytes(ctx, n, crops, k) <= WS_CAP:
        k = (k + 1) // 2
    return k


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's MANIQA scratch, grown on demand and kept apart from its workspace (whose address recorded graphs hold). Growing waits for
    the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_maniqa_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_maniqa_ws"] = None
        ws = ctx.__dict__["_maniqa_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def _origins_tensor(ctx, n: int, h: int, w: int, origins) -> torch.Tensor:
    """The checked origins [n][crops][2] as a device int32 tensor."""
    crop = ctx.__dict__["_maniqa_cfg"]["crop"]
    a = np.asarray(origins, np.int64)
    if a.ndim == 2:
        a = a[None].repeat(n, axis=0)
    if a.ndim != 3 or a.shape[0] != n or a.shape[1] < 1 or a.shape[2] != 2:
        raise _model_module().ManiqaError(f"origins must be [n][crops][2], got {a.shape}")
    if a[..., 0].min() < 0 or a[..., 0].max() > h - crop or a[..., 1].min() < 0 or a[..., 1].max() > w - crop:
        raise _model_module().ManiqaError(f"a crop origin leaves the {h} x {w} image (crop {crop}): y within 0 .. {h - crop}, x within 0 .. {w - crop}")
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(ctx.device, non_blocking=False)


def queue_maniqa(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, origins, out: Optional[torch.Tensor] = None, feat: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_maniqa on the current stream: the top-left h x w of the n images at device address img ([n][rows][pitch] bytes, RGB8). origins: the
    crop origins (y, x), [crops][2] for all images or [n][crops][2]; each is checked against 0 <= y <= h - crop, 0 <= x <= w - crop before
    the upload (ManiqaError). out: a contiguous float64 device tensor of n values - by default the context's own small buffer, whose page-locked
    twin fetch_maniqa() fills. feat: None or a contiguous float32 device tensor [n][crops][N][embed / 2]. ws: by default the context's scratch at
    the size of crops_per_pass(); the results do not depend on it."""
    if not configured(ctx):
        raise ValueError("maniqa: the context has no MANIQA model (instarevive_amd.maniqa.configure)")
    cfg = ctx.__dict__["_maniqa_cfg"]
    if not scorable(h, w, cfg["crop"]):
        raise _model_module().ManiqaError(f"a {h} x {w} image has no {cfg['crop']} x {cfg['crop']} crops (the short side must be above {cfg['crop']})")
    org = _origins_tensor(ctx, n, h, w, origins)
    crops = org.shape[1]
    if out is None:
        buf = ctx.__dict__.get("_maniqa_out")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_maniqa_out"] = (torch.zeros((cap,), dtype=torch.float64, device=ctx.device), torch.zeros((cap,), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n or not out.is_contiguous():
        raise ValueError("queue_maniqa: out must be a contiguous float64 tensor of n values")
    per = (cfg["crop"] // cfg["patch"]) ** 2 * (cfg["embed"] // 2)
    if feat is not None and (feat.dtype != torch.float32 or feat.numel() < n * crops * per or not feat.is_contiguous()):
        raise ValueError("queue_maniqa: feat must be a contiguous float32 tensor of n x crops x tokens x embed / 2 values")
    buf = ws if ws is not None else workspace(ctx, max(ws_bytes(ctx, n, crops, crops_per_pass(ctx, n, crops)), 256))
    ctx.check(ctx.lib.ir_maniqa(ctx.h, ctx.stream(), C.c_void_p(img), rows, pitch, n, h, w, L.ptr(org), crops, L.ptr(out),
                                L.ptr(feat) if feat is not None else None, L.ptr(buf), buf.numel()), "ir_maniqa")
    return out   # org was allocated on this stream: the allocator hands its memory out again only behind the call that reads it


def fetch_maniqa(ctx, n: int) -> List[float]:
    """The scores of the last queue_maniqa(out=None) of n images: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_maniqa_out"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [float(v) for v in host[:n].tolist()]


def score_arrays(ctx, img: np.ndarray, origins=None, name=None) -> float:
    """MANIQA of an HWC uint8 RGB array: upload, one call, wait. origins: None - the configured mode's (uniform, or random keyed by `name`).
    For tools and tests; the pipeline scores in place."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise _model_module().ManiqaError(f"an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    if not configured(ctx):
        raise ValueError("maniqa: the context has no MANIQA model (instarevive_amd.maniqa.configure)")
    cfg = ctx.__dict__["_maniqa_cfg"]
    h, w = img.shape[:2]
    if origins is None:
        origins = crop_origins(h, w, cfg["crop"], cfg["crops"], cfg["mode"], cfg["seed"], name)
    dev = torch.from_numpy(img).to(ctx.device)
    queue_maniqa(ctx, dev.data_ptr(), h, 3 * w, 1, h, w, origins)
    return fetch_maniqa(ctx, 1)[0]


class ManiqaSlot(Pooled):
    """The scores of one staging slot's batch: a float64 device buffer, one value per row, and its page-locked twin. A row is an image of the batch:
    the predictions first, then - when asked for - the stage-1 images. Images whose short side is not above the crop are not launched and score
    NaN. The crops follow the configured mode; the random mode keys each image's draws by its name when plan() gets names, else by its row."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d = self.h = None
        self.shapes: List[Tuple[int, int]] = []
        self.names: List[Optional[str]] = []

    def plan(self, finals: Sequence[Tuple[int, int]], copies: int = 1, names: Optional[Sequence[str]] = None) -> None:
        """finals: the final size (h, w) of every image of the batch; copies: 2 when the stage-1 images are scored as well."""
        if not configured(self.ctx):
            raise ValueError("maniqa: the context has no MANIQA model (instarevive_amd.maniqa.configure)")
        self.shapes = [tuple(int(v) for v in f) for f in finals] * copies
        self.names = (list(names) if names is not None else [str(i) for i in range(len(finals))]) * copies
        rows = len(self.shapes)
        if self.d is None or self.d.numel() < rows:
            cap = max(rows, 16)
            self.d = torch.zeros((cap,), dtype=torch.float64, device=self.ctx.device)
            self.h = torch.zeros((cap,), dtype=torch.float64).pin_memory()

    def reserve(self) -> None:
        """Grow the scratch to what the largest call of this batch needs, before anything of the batch is queued."""
        cfg = self.ctx.__dict__["_maniqa_cfg"]
        n = max(len(self.shapes), 1)
        if any(scorable(h, w, cfg["crop"]) for h, w in self.shapes):
            workspace(self.ctx, max(ws_bytes(self.ctx, n, cfg["crops"], crops_per_pass(self.ctx, n, cfg["crops"])), 256))

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """ir_maniqa of the images [n][h][w][3] (device uint8: the network's output) into rows first .. first + n - 1, on the current stream.
        results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop."""
        cfg = self.ctx.__dict__["_maniqa_cfg"]
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes[first:first + n], results, n):
            gh, gw = self.shapes[first + i]
            out = self.d[first + i:first + k]
            if not scorable(gh, gw, cfg["crop"]):
                out.fill_(float("nan"))
                continue
            org = [crop_origins(gh, gw, cfg["crop"], cfg["crops"], cfg["mode"], cfg["seed"], self.names[first + j]) for j in range(i, k)]
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            queue_maniqa(self.ctx, img, rows, pitch, k - i, gh, gw, org, out)

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's scores on the current stream."""
        rows = len(self.shapes)
        if rows:
            self.h[:rows].copy_(self.d[:rows], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        """(maniqa,) of rows first .. first + count - 1 after the download has completed; NaN for an image without a score."""
        return [(float(v),) for v in self.h[first:first + count].tolist()]
