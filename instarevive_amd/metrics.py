"""PSNR-Y and SSIM-Y of results against ground truth on the device (ir_metrics_y, csrc/metrics.hip): what the reference's evaluate_img.py takes
from pyiqa (`psnr` / `ssim`, test_y_channel=True) and tools/evaluate_pairs.py restates in numpy fp64, computed behind the network from the
uint8 result that is in device memory anyway, so that scoring a run does not mean decoding its own PNGs again.

queue_scores() puts the call on the current stream, ScoreSlot holds the ground-truth images and the scores of one staging slot (page-locked and
device side, like resample.ResizeSlot), GroundTruth finds the ground-truth file of an input and Report writes the per-file CSV and the averages
in evaluate_pairs' format.
"""
import ctypes as C
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled, spans

WINDOW = 11   # the Gaussian window: images below 11 x 11 have no SSIM (the host model raises, ir_metrics_y refuses)


class MetricsError(ValueError):
    pass


def psnr_from_mse(mse: float) -> float:
    """pyiqa's `psnr` at data_range 1 from the unit-scale MSE ir_metrics_y returns (tools/evaluate_pairs.py::psnr_y)."""
    return float(10.0 * math.log10(1.0 / (float(mse) + 1e-8)))


def ws_bytes(n: int, h: int, w: int) -> int:
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_METRICS, n, h, w, 0, 0, 0))


def queue_scores(ctx, a: int, a_rows: int, a_pitch: int, b: int, b_rows: int, b_pitch: int, n: int, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ir_metrics_y on the current stream: the top-left h x w of the n images at device address a ([n][a_rows][a_pitch] bytes, RGB8) against
    those at b. out: a contiguous float64 device tensor of n x 2 values (mse_y, ssim_y) - by default the context's own small buffer, whose
    page-locked twin fetch_scores() fills. The scratch is the context's workspace (stream-ordered like every other call that uses it; a
    caller that has handed its address to a later launch grows it first, see ScoreSlot.reserve)."""
    if out is None:
        buf = ctx.__dict__.get("_scores")
        if buf is None or buf[0].shape[0] < n:
            cap = max(n, 16)
            buf = ctx.__dict__["_scores"] = (torch.zeros((cap, 2), dtype=torch.float64, device=ctx.device), torch.zeros((cap, 2), dtype=torch.float64).pin_memory())
        out = buf[0][:n]
    if out.dtype != torch.float64 or out.numel() < 2 * n or not out.is_contiguous():
        raise ValueError("queue_scores: out must be a contiguous float64 tensor of n x 2 values")
    ws = ctx.workspace(ws_bytes(n, h, w))
    ctx.check(ctx.lib.ir_metrics_y(ctx.h, ctx.stream(), C.c_void_p(a), a_rows, a_pitch, C.c_void_p(b), b_rows, b_pitch, n, h, w, C.c_void_p(out.data_ptr()),
                                   L.ptr(ws), ws.numel()), "ir_metrics_y")
    return out


def fetch_scores(ctx, n: int) -> List[Tuple[float, float]]:
    """The (psnr_y, ssim_y) of the last queue_scores(out=None) of n images: downloads through the page-locked twin and waits for the stream."""
    dev, host = ctx.__dict__["_scores"]
    host[:n].copy_(dev[:n], non_blocking=True)
    torch.cuda.current_stream(ctx.device).synchronize()
    return [(psnr_from_mse(m), float(s)) for m, s in host[:n].tolist()]


def score_arrays(ctx, a: np.ndarray, b: np.ndarray) -> Tuple[float, float]:
    """(psnr_y, ssim_y) of two HWC uint8 RGB arrays of equal size: upload, one call, wait. For tools and tests; the pipeline scores in place."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != b.shape:
        raise MetricsError(f"score_arrays: two HWC uint8 RGB arrays of equal size are needed, got {a.shape} and {b.shape}")
    h, w = a.shape[:2]
    if min(h, w) < WINDOW:
        raise MetricsError("SSIM needs images of at least 11 x 11 pixels")
    da, db = torch.from_numpy(a).to(ctx.device), torch.from_numpy(b).to(ctx.device)
    queue_scores(ctx, da.data_ptr(), h, 3 * w, db.data_ptr(), h, 3 * w, 1, h, w)
    return fetch_scores(ctx, 1)[0]


def check_ground_truth(gts: Sequence[np.ndarray], finals: Sequence[Tuple[int, int]], what: str = "gt", min_edge: int = WINDOW) -> None:
    """Every ground-truth image an HWC uint8 RGB array of its image's final size (h, w); ValueError with both sizes otherwise. min_edge: the
    smallest edge the scorers take (11 for SSIM's window; 31 when LPIPS is scored as well)."""
    if len(gts) != len(finals):
        raise ValueError(f"{what}: {len(gts)} ground-truth images for a batch of {len(finals)} images")
    for i, (g, hw) in enumerate(zip(gts, finals)):
        if not isinstance(g, np.ndarray) or g.dtype != np.uint8 or g.ndim != 3 or g.shape[2] != 3:
            raise ValueError(f"{what}: ground truth {i} must be an HWC uint8 RGB array")
        if tuple(g.shape[:2]) != tuple(hw):
            raise ValueError(f"{what}: ground truth {i} is {g.shape[0]} x {g.shape[1]}, the image's final size is {hw[0]} x {hw[1]}")
        if min(hw) < WINDOW:
            raise ValueError(f"{what}: image {i} is {hw[0]} x {hw[1]}; SSIM needs at least 11 x 11 pixels")
        if min(hw) < min_edge:
            raise ValueError(f"{what}: image {i} is {hw[0]} x {hw[1]}; LPIPS needs at least {min_edge} x {min_edge} pixels")


class ScoreSlot(Pooled):
    """Buffers of one staging slot for batches that are scored: the ground-truth images in a flat page-locked buffer and its device copy (images
    differ in size; the kernel reads bytes, so they are packed without gaps and images of one size form an [n][h][3 w] block), and the scores
    [count][2] (mse_y, ssim_y) with their page-locked twin. All grow on demand and are reused by the next batch of the slot. A batch filled with
    lpips=True is scored by ir_lpips as well (lpips.py; the context's LPIPS weights must be bound): one more double per row, and scores()
    yields (psnr_y, ssim_y, lpips) in place of pairs. A row is an image of the batch: the predictions first, then - filled with copies=2 - the
    stage-1 images, scored against the same ground truth. A batch filled with dists=True is scored by ir_dists as well (dists.py; the context's
    DISTS weights must be bound), queued behind ir_lpips for the same images: one more double per row, which dists_values() yields - DISTS is the
    last value of a score tuple, behind the no-reference scorers', so DistsColumn hands it over there. A pair below 16 pixels on an edge has no
    DISTS on the device: its value is NaN."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h_gt = self.d_gt = None
        self.d_scores = self.h_scores = None
        self.d_lpips = self.h_lpips = None
        self.d_dists = self.h_dists = None
        self.lpips = self.dists = False
        self.h2d_done = None
        self.fresh = False
        self.offsets: List[int] = []
        self.shapes: List[Tuple[int, int]] = []
        self.used = self.rows = 0

    def fill(self, gts: Sequence[np.ndarray], lpips: bool = False, copies: int = 1, dists: bool = False) -> None:
        """Copy the ground-truth images into the page-locked buffer (after the previous upload out of it has completed). copies: 2 when the
        stage-1 images are scored as well."""
        from .resample import _grown
        self.lpips, self.dists, self.rows = bool(lpips), bool(dists), copies * len(gts)
        if self.h2d_done is not None:
            self.h2d_done.synchronize()
            self.h2d_done = None
        self.offsets, self.shapes, at = [], [], 0
        for g in gts:
            self.offsets.append(at)
            self.shapes.append(tuple(g.shape[:2]))
            at += g.size
        self.h_gt = _grown(self.h_gt, at, pinned=True)
        if self.d_gt is None or self.d_gt.numel() < self.h_gt.numel():
            self.d_gt, self.fresh = _grown(None, self.h_gt.numel(), self.ctx.device), True
        self.used = at
        host = self.h_gt.numpy()
        for g, o in zip(gts, self.offsets):
            np.copyto(host[o:o + g.size].reshape(g.shape), g)
        if self.d_scores is None or self.d_scores.shape[0] < 2 * len(gts):
            cap = max(2 * len(gts), 16)
            self.d_scores = torch.zeros((cap, 2), dtype=torch.float64, device=self.ctx.device)
            self.h_scores = torch.zeros((cap, 2), dtype=torch.float64).pin_memory()
        if self.lpips and (self.d_lpips is None or self.d_lpips.shape[0] < 2 * len(gts)):
            cap = max(2 * len(gts), 16)
            self.d_lpips = torch.zeros((cap,), dtype=torch.float64, device=self.ctx.device)
            self.h_lpips = torch.zeros((cap,), dtype=torch.float64).pin_memory()
        if self.dists and (self.d_dists is None or self.d_dists.shape[0] < 2 * len(gts)):
            cap = max(2 * len(gts), 16)
            self.d_dists = torch.zeros((cap,), dtype=torch.float64, device=self.ctx.device)
            self.h_dists = torch.zeros((cap,), dtype=torch.float64).pin_memory()

    def upload(self, stream=None, owner=None):
        """Asynchronous H2D copy of the ground truth on `stream` (default: the current one); stream / owner as in ResizeSlot.upload."""
        if self.fresh and owner is not None and stream is not None:
            stream.wait_stream(owner)
        self.fresh = False
        self.d_gt[:self.used].copy_(self.h_gt[:self.used], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.ctx.device))
        self.h2d_done = ev
        return ev

    def reserve(self) -> None:
        """Grow the context's workspace to what the largest call of this batch may need (all images of one size in one call), and the LPIPS scratch
        (a buffer of its own, lpips.workspace) of a batch filled with lpips=True, before anything of the batch is queued."""
        n = len(self.shapes)
        self.ctx.workspace(max(ws_bytes(n, h, w) for h, w in self.shapes))
        if self.lpips:
            from . import lpips
            lpips.workspace(self.ctx, max(lpips.ws_bytes(n, h, w) for h, w in self.shapes))
        if self.dists:
            from . import dists
            dists.workspace(self.ctx, max(dists.ws_bytes(n, h, w) for h, w in self.shapes))   # 0 for a size below 16 x 16

    def queue(self, first: int, images: torch.Tensor, results: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
        """Score the images [n][h][w][3] (device uint8: the network's output) against the slot's ground truth into score rows first .. first + n - 1,
        on the current stream. results[i], when not None, is image i's resized result [1][th][tw][3] and is scored in place of the crop.
        ir_lpips is queued behind ir_metrics_y for the same images."""
        n, h, w, _ = images.shape
        for i, k, r in spans(self.shapes, results, n):
            gh, gw = self.shapes[i]
            a, a_rows, a_pitch = (images[i].data_ptr(), h, 3 * w) if r is None else (r.data_ptr(), gh, 3 * gw)
            b, out = self.d_gt.data_ptr() + self.offsets[i], slice(first + i, first + k)
            queue_scores(self.ctx, a, a_rows, a_pitch, b, gh, 3 * gw, k - i, gh, gw, self.d_scores[out])
            if self.lpips:
                from .lpips import queue_lpips
                queue_lpips(self.ctx, a, a_rows, a_pitch, b, gh, 3 * gw, k - i, gh, gw, self.d_lpips[out])
            if self.dists:
                from .dists import MIN_EDGE, queue_dists
                if min(gh, gw) < MIN_EDGE:
                    self.d_dists[out].fill_(float("nan"))
                else:
                    queue_dists(self.ctx, a, a_rows, a_pitch, b, gh, 3 * gw, k - i, gh, gw, self.d_dists[out])

    def download(self) -> None:
        """Asynchronous D2H copy of the batch's score rows on the current stream."""
        self.h_scores[:self.rows].copy_(self.d_scores[:self.rows], non_blocking=True)
        if self.lpips:
            self.h_lpips[:self.rows].copy_(self.d_lpips[:self.rows], non_blocking=True)
        if self.dists:
            self.h_dists[:self.rows].copy_(self.d_dists[:self.rows], non_blocking=True)

    def scores(self, first: int, count: int) -> List[Tuple[float, ...]]:
        """(psnr_y, ssim_y) of rows first .. first + count - 1 after the download has completed; (psnr_y, ssim_y, lpips) for a batch filled with
        lpips=True."""
        pairs = [(psnr_from_mse(m), float(s)) for m, s in self.h_scores[first:first + count].tolist()]
        if not self.lpips:
            return pairs
        return [p + (float(v),) for p, v in zip(pairs, self.h_lpips[first:first + count].tolist())]

    def dists_values(self, first: int, count: int) -> List[float]:
        """DISTS of rows first .. first + count - 1 of a batch filled with dists=True, after the download has completed."""
        return [float(v) for v in self.h_dists[first:first + count].tolist()]


class DistsColumn:
    """The place of DISTS in a score tuple: the last one, behind the no-reference scorers'. The values are ScoreSlot's (it queues ir_dists with
    its own calls and downloads them with its own rows); this object only stands where they are read."""

    def __init__(self, slot: ScoreSlot):
        self.slot = slot

    def reserve(self) -> None:
        pass

    def queue(self, first, images, results=None) -> None:
        pass

    def download(self) -> None:
        pass

    def scores(self, first: int, count: int) -> List[Tuple[float]]:
        return [(v,) for v in self.slot.dists_values(first, count)]


class GroundTruth:
    """The ground-truth file of an input, by the rules prompts.caption_file uses for captions: `gt_dir/<path relative to input_root>` with any
    image extension list_image_files accepts first, then `gt_dir/<file stem>.*` (a flat folder). Unlike a caption, a ground truth is not
    optional: a missing file and an ambiguous one (two extensions of one stem) raise MetricsError naming the input."""

    def __init__(self, gt_dir: str, input_root: Optional[str] = None):
        if not os.path.isdir(gt_dir):
            raise MetricsError(f"--gt {gt_dir} is not a directory")
        self.gt_dir, self.input_root = gt_dir, input_root

    @staticmethod
    def _matches(folder: str, stem: str) -> List[str]:
        from .utils import IMAGE_EXTENSIONS
        try:
            names = sorted(os.listdir(folder))
        except OSError:
            return []
        return [os.path.join(folder, nm) for nm in names
                if os.path.splitext(nm)[0] == stem and os.path.splitext(nm)[1].lower() in IMAGE_EXTENSIONS and os.path.isfile(os.path.join(folder, nm))]

    def path(self, image_path: str) -> str:
        stem = os.path.splitext(os.path.basename(image_path))[0]
        folders = []
        if self.input_root is not None:
            rel = os.path.relpath(image_path, self.input_root)
            if not rel.startswith(".."):
                folders.append(os.path.join(self.gt_dir, os.path.dirname(rel)))
        if os.path.normpath(self.gt_dir) not in [os.path.normpath(f) for f in folders]:   # a top-level input: both rules name one folder
            folders.append(self.gt_dir)
        for folder in folders:
            found = self._matches(folder, stem)
            if len(found) > 1:
                raise MetricsError(f"ground truth of {image_path} is ambiguous: {', '.join(found)}")
            if found:
                return found[0]
        raise MetricsError(f"no ground truth for {image_path} under {self.gt_dir} (looked for {stem}.* with an image extension)")

    def load(self, image_path: str):
        """The ground truth of an input as a PIL RGB image."""
        from PIL import Image
        return Image.open(self.path(image_path)).convert("RGB")


class Report:
    """Per-file scores of a run: one CSV row per file (`file,psnr_y,ssim_y`, the values with every digit) and the averages in evaluate_pairs'
    format (`psnr: %.5f`, `ssim: %.5f`). A report made with lpips=True carries LPIPS as well: every add() then takes the third value, the header
    is `file,psnr_y,ssim_y,lpips` and the averages gain `lpips: %.5f` after `ssim`. niqe=True appends the no-reference NIQE (niqe.py) as the last
    column and the last average line (`niqe: %.5f`); clipiqa=True appends CLIP-IQA (clipiqa.py) behind it (`clipiqa: %.5f`, evaluate_img.py's
    key), musiq=True appends MUSIQ (musiq.py) behind that (`musiq: %.5f`), maniqa=True MANIQA (maniqa.py) behind that (`maniqa: %.5f`). The
    full column order is `file,psnr_y,ssim_y,lpips,niqe,clipiqa,musiq,maniqa`; absent metrics are left out. paired=False (a run without ground truth) carries the
    no-reference columns alone: `file,niqe`, `file,clipiqa`, `file,musiq`, `file,maniqa`, `file,niqe,clipiqa` and so on. HEADERS lists
    the headers without the MANIQA column, HEADERS_MANIQA those with it. dists=True (a paired report only) appends DISTS (dists.py) as the very
    last column and average line (`dists: %.5f`): the full order ends `...,musiq,maniqa,dists`; HEADERS_DISTS lists those headers. ilniqe=True puts
    IL-NIQE (ilniqe.py) right behind NIQE's place (`...,niqe,ilniqe,clipiqa,...`, `ilniqe: %.5f`); a report without it is what it was.
    topiq_nr=True puts TOPIQ-NR (topiq.py) behind MANIQA's place and before DISTS's (`...,musiq,maniqa,topiq_nr,dists`, `topiq_nr: %.5f`);
    HEADERS_TOPIQ lists those headers, and a report without the column is what it was."""
    HEADER = "file,psnr_y,ssim_y"
    HEADER_LPIPS = HEADER + ",lpips"
    HEADER_NIQE = "file,niqe"
    HEADERS = tuple(p + n + c + m for p in (HEADER, HEADER_LPIPS, "file") for n in ("", ",niqe") for c in ("", ",clipiqa") for m in ("", ",musiq")
                    if p != "file" or n or c or m)
    HEADERS_MANIQA = tuple(h + ",maniqa" for h in HEADERS + ("file",))
    HEADERS_DISTS = tuple(h + ",dists" for h in HEADERS + HEADERS_MANIQA if h.startswith("file,psnr_y,ssim_y"))
    HEADERS_TOPIQ = tuple(h[:-len(",dists")] + ",topiq_nr,dists" if h.endswith(",dists") else h + ",topiq_nr" for h in HEADERS + HEADERS_MANIQA + HEADERS_DISTS + ("file",))

    def __init__(self, path: Optional[str] = None, lpips: bool = False, niqe: bool = False, paired: bool = True, clipiqa: bool = False,
                 musiq: bool = False, maniqa: bool = False, dists: bool = False, ilniqe: bool = False, topiq_nr: bool = False):
        self.ilniqe, self.topiq_nr = bool(ilniqe), bool(topiq_nr)
        self.path, self.rows, self.lpips, self.niqe, self.paired, self.clipiqa = path, [], bool(lpips), bool(niqe), bool(paired), bool(clipiqa)
        self.musiq, self.maniqa, self.dists = bool(musiq), bool(maniqa), bool(dists)
        if self.dists and not self.paired:
            raise MetricsError("Report: DISTS is a paired score; a report without paired scores cannot carry it")
        if not self.paired and (self.lpips or not (self.niqe or self.ilniqe or self.clipiqa or self.musiq or self.maniqa or self.topiq_nr)):
            raise MetricsError("Report: a report without paired scores carries NIQE, CLIP-IQA, MUSIQ, MANIQA and / or TOPIQ-NR and nothing else")
        self.keys = ((("psnr", "ssim") + (("lpips",) if self.lpips else ()) if self.paired else ()) + (("niqe",) if self.niqe else ()) + (("ilniqe",) if self.ilniqe else ())
                     + (("clipiqa",) if self.clipiqa else ()) + (("musiq",) if self.musiq else ()) + (("maniqa",) if self.maniqa else ()) + (("topiq_nr",) if self.topiq_nr else ())
                     + (("dists",) if self.dists else ()))

    def add(self, name: str, psnr: Optional[float] = None, ssim: Optional[float] = None, lpips: Optional[float] = None, niqe: Optional[float] = None,
            clipiqa: Optional[float] = None, musiq: Optional[float] = None, maniqa: Optional[float] = None, dists: Optional[float] = None, ilniqe: Optional[float] = None, topiq_nr: Optional[float] = None) -> None:
        if (topiq_nr is not None) != self.topiq_nr:
            raise MetricsError("Report.add: a TOPIQ-NR value is needed by a report made with topiq_nr=True and by no other")
        if (ilniqe is not None) != self.ilniqe:
            raise MetricsError("Report.add: an IL-NIQE value is needed by a report made with ilniqe=True and by no other")
        if (lpips is not None) != self.lpips:
            raise MetricsError("Report.add: an LPIPS value is needed by a report made with lpips=True and by no other")
        if (niqe is not None) != self.niqe:
            raise MetricsError("Report.add: a NIQE value is needed by a report made with niqe=True and by no other")
        if (clipiqa is not None) != self.clipiqa:
            raise MetricsError("Report.add: a CLIP-IQA value is needed by a report made with clipiqa=True and by no other")
        if (musiq is not None) != self.musiq:
            raise MetricsError("Report.add: a MUSIQ value is needed by a report made with musiq=True and by no other")
        if (maniqa is not None) != self.maniqa:
            raise MetricsError("Report.add: a MANIQA value is needed by a report made with maniqa=True and by no other")
        if (dists is not None) != self.dists:
            raise MetricsError("Report.add: a DISTS value is needed by a report made with dists=True and by no other")
        if (psnr is not None) != self.paired or (ssim is not None) != self.paired:
            raise MetricsError("Report.add: PSNR and SSIM are needed by a report with paired scores and by no other")
        given = dict(psnr=psnr, ssim=ssim, lpips=lpips, niqe=niqe, ilniqe=ilniqe, clipiqa=clipiqa, musiq=musiq, maniqa=maniqa, topiq_nr=topiq_nr, dists=dists)
        self.rows.append((str(name),) + tuple(float(given[k]) for k in self.keys))

    def add_scores(self, name: str, scores: Sequence[float]) -> None:
        """add() with the values in the report's own column order: a score tuple of process_stream()."""
        if len(scores) != len(self.keys):
            raise MetricsError(f"Report.add_scores: {len(scores)} values for the columns {', '.join(self.keys)}")
        self.add(name, **dict(zip(self.keys, scores)))

    def unscored(self, scores: Sequence[float]) -> Optional[str]:
        """For a score tuple in the report's own column order: the no-reference column whose value is NaN - the image has no such score -
        "niqe" before "clipiqa" before "musiq" before "maniqa" before "topiq_nr" - or "dists" behind them (a pair below 16 pixels on an edge); None when the tuple
        can be added."""
        for k in ("niqe", "ilniqe", "clipiqa", "musiq", "maniqa", "topiq_nr", "dists"):
            if k in self.keys and scores[self.keys.index(k)] != scores[self.keys.index(k)]:
                return k
        return None

    def header(self) -> str:
        return ",".join(("file",) + tuple({"psnr": "psnr_y", "ssim": "ssim_y"}.get(k, k) for k in self.keys))

    def averages(self) -> dict:
        if not self.rows:
            return {}
        return {k: sum(r[i + 1] for r in self.rows) / len(self.rows) for i, k in enumerate(self.keys)}

    def average_lines(self) -> List[str]:
        return [f"{k}: {v:.5f}" for k, v in self.averages().items()]

    def csv_lines(self) -> List[str]:
        import csv
        import io
        buf = io.StringIO()
        wr = csv.writer(buf, lineterminator="\n")
        for row in sorted(self.rows):
            wr.writerow([row[0]] + [repr(v) for v in row[1:]])
        return [self.header()] + buf.getvalue().splitlines()

    def write(self) -> List[str]:
        """Write the CSV (when the report has a path) and return the average lines."""
        if self.path:
            os.makedirs(os.path.dirname(self.path) or ".", exist_ok=True)
            with open(self.path, "w") as f:
                f.write("\n".join(self.csv_lines()) + "\n")
        return self.average_lines()


def read_report(path: str) -> dict:
    """{file: (psnr_y, ssim_y)} of a CSV that Report wrote; {file: (psnr_y, ssim_y, lpips)} of one with the LPIPS column; with the NIQE column
    that value follows, with the CLIP-IQA, MUSIQ, MANIQA and TOPIQ-NR columns those values follow, with the DISTS column that value comes last; a `file,niqe` report gives {file: (niqe,)}."""
    import csv
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    head = [c for c in rows[0] if c != "ilniqe"] if rows else []   # the IL-NIQE column may stand in any report
    if not rows or (",".join(head) not in Report.HEADERS + Report.HEADERS_MANIQA + Report.HEADERS_DISTS + Report.HEADERS_TOPIQ and rows[0] not in (["file", "ilniqe"], ["file", "ilniqe", "topiq_nr"])):
        raise MetricsError(f"{path}: not a metrics report")
    return {r[0]: tuple(float(v) for v in r[1:len(rows[0])]) for r in rows[1:]}
