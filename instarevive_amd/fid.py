"""FID on the device: the per-image Inception-v3 features (ir_fid_features, csrc/fid.hip) and the set-level half in fp64 on the host.
tools/evaluate_fid.py restates the network, the two resizes and the Frechet distance and is the definition; this module loads the user's
weights (they do not ship with the project), binds them (ir_fid_configure), queues the device call beside dists.queue_dists() and keeps the
features of a run until its end: FID is a statistic of the whole set, so there is no per-file value.

FeatureSet, statistics(), frechet_distance(), load_stats() and merge() are evaluate_fid.py's own, so that the tool and the library cannot drift.
"""
import ctypes as C
import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled

SIZE, DIM, BLOCK_CHANNELS = L.FID_SIZE, L.FID_DIM, L.FID_BLOCK_CHANNELS
MIN_EDGE = 2   # a limit of the library (ir_fid_features refuses below it)
MODES = {"clean": L.FID_RESIZE_CLEAN, "legacy": L.FID_RESIZE_LEGACY}


def _evaluate_fid():
    """tools/evaluate_fid.py as a module: the network's table, key names, loader and the set-level arithmetic are defined there once."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import evaluate_fid
    return evaluate_fid


_E = _evaluate_fid()
FidError = _E.FidError
FeatureSet = _E.FeatureSet
statistics = _E.statistics
frechet_distance = _E.frechet_distance
load_stats = _E.load_stats
merge = _E.merge
rank_deficient_note = _E.rank_deficient_note
tensor_names = _E.tensor_names
BLOCKS, BLOCK_WIDTH = _E.BLOCKS, _E.BLOCK_WIDTH


def load_weights(model) -> Dict[str, torch.Tensor]:
    """The tensors ir_fid_configure binds, from a pytorch-fid / torchvision state dict (or its .pth) or an .npz (or dict) in ir_fid_configure's
    names. The same KeyError / ValueError as the host model for a missing key or a shape that is not Inception-v3's."""
    return _E.load_weights(model)


def configure(ctx, model) -> None:
    """Upload the weights and bind them. Replaces an earlier binding of the context."""
    for k, v in load_weights(model).items():
        ctx.upload(k, v)
    ctx.check(ctx.lib.ir_fid_configure(ctx.h), "ir_fid_configure")
    ctx.__dict__["_fid_ready"] = True


def configured(ctx) -> bool:
    return bool(ctx.__dict__.get("_fid_ready"))


def resize_plan(h: int, w: int, mode="clean") -> np.ndarray:
    """ir_fid_resize_plan's tables as bytes in an 8-byte aligned array (host only, needs no GPU)."""
    lib = L.load_library()
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    nbytes = int(lib.ir_fid_resize_plan_bytes(h, w, m))
    if nbytes <= 0:
        raise FidError(f"ir_fid_resize_plan: bad size {h} x {w} or mode {mode!r}")
    buf = np.zeros((nbytes + 7) // 8, np.int64)
    if lib.ir_fid_resize_plan(h, w, m, C.c_void_p(buf.ctypes.data), nbytes) != 0:
        raise FidError("ir_fid_resize_plan failed")
    return buf.view(np.uint8)[:nbytes]


def plan_tables(plan: np.ndarray, h: int, w: int, mode="clean") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(x bounds [299][2], x coefficients [299][kx], y bounds, y coefficients) of a resize_plan(): the layout the header states."""
    b = np.ascontiguousarray(plan)
    xb = b[:2 * SIZE * 4].view(np.int32).reshape(SIZE, 2)
    yb = b[2 * SIZE * 4:4 * SIZE * 4].view(np.int32).reshape(SIZE, 2)
    k = b[4 * SIZE * 4 + 8:].view(np.float64)
    if (isinstance(mode, str) and mode == "legacy") or mode == L.FID_RESIZE_LEGACY:
        kx = ky = 2
    else:
        kx, ky = _E.clean_tables(w)[1].shape[1], _E.clean_tables(h)[1].shape[1]
    assert k.size == SIZE * (kx + ky), (k.size, kx, ky)
    return xb, k[:SIZE * kx].reshape(SIZE, kx), yb, k[SIZE * kx:].reshape(SIZE, ky)


def device_tables(ctx, h: int, w: int, mode="clean") -> torch.Tensor:
    """The tables of one size on the device, kept per context (a run sees few sizes)."""
    cache = ctx.__dict__.setdefault("_fid_tables", {})
    key = (h, w, mode)
    if key not in cache:
        if len(cache) >= 64:
            torch.cuda.synchronize(ctx.device)   # a call queued earlier may still read a table
            cache.clear()
        cache[key] = torch.from_numpy(resize_plan(h, w, mode).copy()).to(ctx.device)
    return cache[key]


def ws_bytes(n: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_FID, n, 0, 0, 0, 0, 0))


def workspace(ctx, nbytes: int) -> torch.Tensor:
    """The context's FID scratch, grown on demand. Growing waits for the device first: a call queued earlier may still use the old buffer."""
    ws = ctx.__dict__.get("_fid_ws")
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            torch.cuda.synchronize(ctx.device)
        ctx.__dict__["_fid_ws"] = None
        ws = ctx.__dict__["_fid_ws"] = torch.empty(int(nbytes), dtype=torch.uint8, device=ctx.device)
    return ws


def queue_fid(ctx, img: int, rows: int, pitch: int, n: int, h: int, w: int, mode="clean", out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
              block_means: Optional[torch.Tensor] = None, resized: Optional[torch.Tensor] = None, slot: int = 0) -> torch.Tensor:
    """ir_fid_features on the current stream: the top-left h x w of the n images at device address img ([n][rows][pitch] bytes, RGB8).
    out: a contiguous float64 device tensor of n x 2048 values - by default the context's own buffer `slot` (0: results, 1: ground truth), whose
    page-locked twin fetch_fid() fills. ws: the scratch; by default a grow-only buffer of the context. block_means: float64 [n][10304] or None;
    resized: float32 [n][299][299][3] or None."""
    if out is None:
        bufs = ctx.__dict__.setdefault("_fid_out", {})
        buf = bufs.get(slot)
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 8)
            buf = bufs[slot] = (torch.zeros((cap, DIM), dtype=torch.float64, device=ctx.device), torch.zeros((cap, DIM), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < n * DIM or not out.is_contiguous():
        raise ValueError("queue_fid: out must be a contiguous float64 tensor of n x 2048 values")
    if block_means is not None and (block_means.dtype != torch.float64 or block_means.numel() < n * BLOCK_CHANNELS or not block_means.is_contiguous()):
        raise ValueError("queue_fid: block_means must be a contiguous float64 tensor of n x 10304 values")
    if resized is not None and (resized.dtype != torch.float32 or resized.numel() < n * SIZE * SIZE * 3 or not resized.is_contiguous()):
        raise ValueError("queue_fid: resized must be a contiguous float32 tensor of n x 299 x 299 x 3 values")
    if ws is None:
        ws = workspace(ctx, ws_bytes(n))
    tables = device_tables(ctx, h, w, mode)
    ctx.check(ctx.lib.ir_fid_features(ctx.h, ctx.stream(), C.c_void_p(img), rows, pitch, n, h, w, MODES[mode], L.ptr(tables), C.c_void_p(out.data_ptr()),
                                      None if block_means is None else C.c_void_p(block_means.data_ptr()),
                                      None if resized is None else C.c_void_p(resized.data_ptr()), L.ptr(ws), ws.numel()), "ir_fid_features")
    return out


def fetch_fid(ctx, n: int, slot: int = 0) -> np.ndarray:
    """[n][2048] float64: the features of the last queue_fid(out=None, slot=slot) of n images; downloads through the page-locked twin and waits."""
    dev, host = ctx.__dict__["_fid_out"][slot]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return host[:n].numpy().copy()


def fid_arrays(ctx, img: np.ndarray, mode="clean") -> np.ndarray:
    """[1][2048] features of one HWC uint8 RGB array: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise FidError(f"fid_arrays: an HWC uint8 RGB array is needed, got {img.shape} {img.dtype}")
    h, w = img.shape[:2]
    if min(h, w) < MIN_EDGE:
        raise FidError(f"FID's features are taken from {MIN_EDGE} x {MIN_EDGE} pixels")
    d = torch.from_numpy(img).to(ctx.device)
    queue_fid(ctx, d.data_ptr(), h, 3 * w, 1, h, w, mode)
    return fetch_fid(ctx, 1)


def features_of(ctx, images: List[np.ndarray], mode="clean") -> np.ndarray:
    """[N][2048] features of a list of images of any sizes, one call each."""
    return np.concatenate([fid_arrays(ctx, im, mode) for im in images]) if images else np.zeros((0, DIM))


class FidSlot(Pooled):
    """The features of one staging slot's batch: a float64 device buffer [n][2048] for the predictions and, when the batch has ground truth, one
    for the ground-truth images (read from the paired slot's device copy), each with a page-locked twin. FID is a statistic of the whole set, so
    the rows are no score columns: pipeline._Batch hands them over beside the scores."""
    def __init__(self, ctx):
        self.ctx = ctx
        self.d = self.h = self.d_gt = self.h_gt = None
        self.shapes: List[Tuple[int, int]] = []
        self.sc, self.mode = None, "clean"

    def plan(self, finals, mode="clean", sc=None) -> None:
        """finals: the final size (h, w) of every image of the batch; sc: the batch's metrics.ScoreSlot when its ground truth joins the set."""
        if not configured(self.ctx):
            raise ValueError("fid: no Inception weights are bound to the context (instarevive_amd.fid.configure)")
        if mode not in MODES:
            raise ValueError(f"fid: resize mode {mode!r} (clean or legacy)")
        self.shapes = [tuple(int(v) for v in f) for f in finals]
        if any(min(s) < MIN_EDGE for s in self.shapes):
            raise ValueError(f"fid: FID's features are taken from {MIN_EDGE} x {MIN_EDGE} pixels, got {self.shapes}")
        self.mode, self.sc = mode, sc
        n = len(self.shapes)
        if self.d is None or self.d.shape[0] < n:
            cap = max(n, 8)
            self.d = torch.zeros((cap, DIM), dtype=torch.float64, device=self.ctx.device)
            self.h = torch.zeros((cap, DIM), dtype=torch.float64).pin_memory()
        if sc is not None and (self.d_gt is None or self.d_gt.shape[0] < n):
            cap = max(n, 8)
            self.d_gt = torch.zeros((cap, DIM), dtype=torch.float64, device=self.ctx.device)
            self.h_gt = torch.zeros((cap, DIM), dtype=torch.float64).pin_memory()

    def reserve(self) -> None:
        """Grow the scratch and upload the resize tables of the batch's sizes before anything of the batch is queued."""
        workspace(self.ctx, ws_bytes(len(self.shapes)))
        for h, w in set(self.shapes) | (set(self.sc.shapes) if self.sc is not None else set()):
            device_tables(self.ctx, h, w, self.mode)

    def queue(self, first: int, images: torch.Tensor, results=None) -> None:
        """ir_fid_features of the predictions [n][h][w][3] (rows from `first` 0; the stage-1 images do not enter the set) on the current stream,
        then of the slot's ground truth. results[i], when not None, is image i's resized result and is taken in place of the crop."""
        from .slots import spans
        if first != 0:
            return
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes, results, n):
            gh, gw = self.shapes[i]
            img, rows, pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            queue_fid(self.ctx, img, rows, pitch, k - i, gh, gw, self.mode, self.d[i:k])
        if self.sc is not None:
            for i, k, _ in spans(self.sc.shapes, None, n):
                gh, gw = self.sc.shapes[i]
                queue_fid(self.ctx, self.sc.d_gt.data_ptr() + self.sc.offsets[i], gh, 3 * gw, k - i, gh, gw, self.mode, self.d_gt[i:k])

    def download(self) -> None:
        n = len(self.shapes)
        self.h[:n].copy_(self.d[:n], non_blocking=True)
        if self.sc is not None:
            self.h_gt[:n].copy_(self.d_gt[:n], non_blocking=True)

    def features(self) -> Dict[str, Optional[np.ndarray]]:
        """{"fid": [n][2048], "fid_gt": [n][2048] or None} after the download has completed."""
        n = len(self.shapes)
        return {"fid": self.h[:n].numpy().copy(), "fid_gt": self.h_gt[:n].numpy().copy() if self.sc is not None else None}


def check_flags(args, reference: bool):
    """The refusals the command lines share, before anything is loaded: (weights, stats) of --fid_model / --fid_stats, or (None, None) without
    --fid_model. reference: the run has ground truth (--gt, or --degrade, whose inputs are the ground truth)."""
    model, stats = getattr(args, "fid_model", None), getattr(args, "fid_stats", None)
    if not model:
        for flag in ("fid_stats", "fid_features_out"):
            if getattr(args, flag, None):
                raise SystemExit(f"--{flag} needs --fid_model (the Inception weights of FID)")
        if getattr(args, "fid_resize", "clean") != "clean":
            raise SystemExit("--fid_resize needs --fid_model (the Inception weights of FID)")
        return None, None
    if not (reference or stats):
        raise SystemExit("--fid_model needs a reference set: give --gt (or --degrade), or --fid_stats FILE.npz")
    if getattr(args, "shard_tiles", False):
        raise SystemExit("--fid_model is not offered together with --shard_tiles (the assembled frame of the tile-sharded path is not scored on the device)")
    for flag in ("fid_model", "fid_stats"):
        if getattr(args, flag, None) and not os.path.isfile(getattr(args, flag)):
            raise SystemExit(f"--{flag} {getattr(args, flag)}: no such file")
    try:
        loaded = load_stats(stats) if stats else None
    except Exception as e:
        raise SystemExit(f"--fid_stats {stats}: {e}")
    try:
        return load_weights(model), loaded
    except Exception as e:   # KeyError / ValueError of the loader; a file torch cannot unpickle raises its own kinds
        raise SystemExit(f"--fid_model {model}: {e}")


class Run:
    """The FID of one command-line run: every rank keeps the features of its files (and of their ground truth, unless `stats` is the reference),
    writes them to its own file, and after the group's barrier rank 0 merges all files and makes the one value. No collective carries data."""

    def __init__(self, path: str, stats=None, rank: int = 0, world: int = 1):
        self.path, self.stats, self.rank, self.world = path, stats, rank, world
        self.pred, self.gt, self.left_out = FeatureSet(), FeatureSet(), 0

    @staticmethod
    def default_path(output_dir: str, given: Optional[str] = None) -> str:
        return given or os.path.join(output_dir, "fid_features.npz")

    def rank_path(self, k: int) -> str:
        if self.world == 1:
            return self.path
        root, ext = os.path.splitext(self.path)
        return f"{root}.rank{k}{ext or '.npz'}"

    def add(self, names, extra) -> None:
        """names: the saved files of a batch; extra: the batch's features dict, or None for a batch that did not enter the set."""
        if extra is None:
            self.left_out += len(names)
            return
        for i, n in enumerate(names):
            self.pred.add(n, extra["fid"][i])
            if self.stats is None and extra["fid_gt"] is not None:
                self.gt.add(n, extra["fid_gt"][i])

    def finish(self, log=print) -> Optional[float]:
        """Write this rank's file, wait for the others, and on rank 0 merge, log the `fid:` line and write it to fid.txt beside the features."""
        mine = self.rank_path(self.rank)
        os.makedirs(os.path.dirname(mine) or ".", exist_ok=True)
        self.pred.save(mine, gt_names=np.array(self.gt.names, dtype=np.str_), gt_features=self.gt.features)
        log(f"[rank {self.rank}] --fid_model: {len(self.pred)} files entered the set, {self.left_out} did not"
            + (" (their saved image is not the device's image, or they have no ground truth)" if self.left_out else "") + f" -> {mine}")
        if self.world > 1:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                dist.barrier()
        if self.rank != 0:
            return None
        files = [self.rank_path(k) for k in range(self.world)]
        pred = merge([FeatureSet.load(f) for f in files])
        try:
            if self.stats is not None:
                ref_n, stats = None, self.stats
            else:
                ref = merge([FeatureSet.load(f, "gt_features", "gt_names") for f in files])
                ref_n, stats = len(ref), statistics(ref.features)
            value = frechet_distance(*statistics(pred.features), *stats)
        except FidError as e:
            log(f"fid: not computed ({e})")
            return None
        note = rank_deficient_note(min(len(pred), ref_n) if ref_n is not None else len(pred))
        if note:
            log(note)
        line = f"fid: {value:.5f}"
        log(line)
        with open(os.path.join(os.path.dirname(self.path) or ".", "fid.txt"), "w") as f:
            f.write(line + "\n")
        return value
