"""The command line's resizes on the device (ir_resample_u8, csrc/resample.hip): the bicubic enlargements ahead of the network (--sr_scale,
auto_resize: test_scripts/inference.py:263-291) and the LANCZOS resize of the result back to the LQ size (:323-346). Both are Pillow's 8-bit
separable resampling - integer arithmetic with fixed rounding - so the device's bytes are Pillow's and the saved files hold the same pixels.

job_geometry() is the size arithmetic of a file without its pixels, Plans keeps the coefficient tables (made on the host: they need double
sin()) per size pair, ResizeSlot the page-locked and device buffers of decoded files and resized results of one staging slot.

With --degrade the decoded files are ground truth: ResizeSlot.fill() packs every file's blur kernel and noise field (degrade.Params) behind
the images, ResizeSlot.degrade() turns them into LQ images on the device (ir_degrade) between the upload and to_network(), which then reads
those.

--center_crop gpu: crop_geometry() is the size arithmetic of utils.center_crop_arr (BOX halvings, the bicubic resize of the short edge, the
central window). ResizeSlot runs such a geometry as a chain of ir_resample_u8 calls whose last step is ir_resample_u8_window - the window alone,
straight into the network input; with --degrade the crop is made first and is what is degraded.
"""
import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .slots import Pooled

BICUBIC, LANCZOS, BOX = L.RESAMPLE_BICUBIC, L.RESAMPLE_LANCZOS, L.RESAMPLE_BOX


class Geometry(NamedTuple):
    chain: tuple      # sizes (w, h) the decoded file is bicubic-resized to, in order: none, one (--sr_scale or auto_resize) or two (both)
    valid_hw: tuple   # (h, w) of the image the network sees, before the pad
    net_hw: tuple     # (h, w) of the network input: valid_hw padded to multiples of 64
    lq_size: tuple    # (w, h) after --sr_scale: the size of the saved result
    lanczos: Optional[tuple]   # lq_size when the result is resized back to it (auto_resize enlarged the file), else None
    # a centre crop (crop_geometry) alone sets the rest: the chain may then be longer than two, a step of equal size is skipped, and the network
    # sees the window of valid_hw at `crop` of the last size
    filters: tuple = ()            # the filter of every chain step (BICUBIC / BOX); empty: all BICUBIC
    crop: Optional[tuple] = None   # (top, left) of the window in the chain's last size


def crop_geometry(size: Tuple[int, int], sr_scale: float, image_size: int) -> Geometry:
    """What inference.py's decode_job() with --use_center_crop (and eval_batch.py) does to the sizes of a decoded file of `size` = (w, h): the
    --sr_scale bicubic, then utils.center_crop_arr - the same expressions in the same floating-point order (math.ceil(edge * sr_scale);
    floor(edge * 0.5) while the short edge is at least twice the target; round(edge * (image_size / short)); the central window)."""
    w, h = (int(v) for v in size)
    s = int(image_size)
    chain, filters = [], []
    if sr_scale != 1:
        w, h = (math.ceil(edge * sr_scale) for edge in (w, h))
        chain.append((w, h))
        filters.append(BICUBIC)
    while min(w, h) >= 2 * s:
        w, h = (int(math.floor(edge * 0.5)) for edge in (w, h))
        chain.append((w, h))
        filters.append(BOX)
    scale = s / min(w, h)
    w, h = (int(round(edge * scale)) for edge in (w, h))
    chain.append((w, h))
    filters.append(BICUBIC)
    return Geometry(tuple(chain), (s, s), (s, s), (s, s), None, tuple(filters), ((h - s) // 2, (w - s) // 2))


def job_geometry(size: Tuple[int, int], sr_scale: float, tiled: bool, tile_size: int) -> Geometry:
    """What inference.py's read_job() does to the sizes of a decoded file of `size` = (w, h), without --use_center_crop: the same expressions
    in the same floating-point order (math.ceil(edge * sr_scale); utils.auto_resize's ceil(edge * (target / short)))."""
    w, h = (int(v) for v in size)
    chain = []
    if sr_scale != 1:
        w, h = (math.ceil(edge * sr_scale) for edge in (w, h))
        chain.append((w, h))
    lq = (w, h)
    target = tile_size if tiled else 512
    short = min(w, h)
    if short < target:
        w, h = (int(math.ceil(edge * (target / short))) for edge in (w, h))
        chain.append((w, h))
    return Geometry(tuple(chain), (h, w), (h + -h % 64, w + -w % 64), lq, lq if lq != (w, h) else None)


class ResizeJob(NamedTuple):
    """One image of a process(resize=...) batch: the decoded file (HWC uint8 RGB) - or a jpeg_decode.JpegSource / png_decode.PngSource, a JPEG or
    PNG file the device decodes into the place the pixels would have been copied to - and its job_geometry()."""
    raw: np.ndarray
    geo: Geometry


def host_plan(in_h: int, in_w: int, out_h: int, out_w: int, flt: int) -> torch.Tensor:
    """ir_resample_plan's tables as a page-locked int32 tensor (pure host code)."""
    lib = L.load_library()
    nbytes = int(lib.ir_resample_plan_bytes(in_h, in_w, out_h, out_w, flt))
    if nbytes == 0:
        raise ValueError(f"no resampling plan for {in_h} x {in_w} -> {out_h} x {out_w}, filter {flt}")
    plan = torch.empty(nbytes // 4, dtype=torch.int32)
    if torch.cuda.is_available():
        plan = plan.pin_memory()
    if lib.ir_resample_plan(in_h, in_w, out_h, out_w, flt, C.c_void_p(plan.data_ptr()), nbytes) != 0:
        raise RuntimeError("ir_resample_plan refused a size it gave a byte count for")
    return plan


class Plans:
    """Plan cache of a context, keyed by (in_h, in_w, out_h, out_w, filter) and bounded like the staging pool: each entry holds the plan in
    page-locked memory and its device copy, uploaded asynchronously on the stream that is current at the first use - the stream of the
    resampling calls themselves, so no wait is needed. A folder of equal-sized files plans once."""
    LIMIT = 64

    def __init__(self, ctx):
        self.ctx, self.pool = ctx, {}

    @staticmethod
    def of(ctx) -> "Plans":
        return ctx.__dict__.setdefault("_resample_plans", Plans(ctx))

    def get(self, in_h, in_w, out_h, out_w, flt) -> torch.Tensor:
        key = (in_h, in_w, out_h, out_w, flt, torch.cuda.current_stream(self.ctx.device).cuda_stream)
        if key not in self.pool:
            if len(self.pool) >= self.LIMIT:   # a copy still queued keeps its memory: torch frees both sides in stream order
                self.pool.pop(next(iter(self.pool)))
            host = host_plan(in_h, in_w, out_h, out_w, flt)
            self.pool[key] = (host, host.to(self.ctx.device, non_blocking=True))
        return self.pool[key][1]


def ws_bytes(n: int, in_h: int, in_w: int, out_h: int, out_w: int) -> int:
    """Workspace of one ir_resample_u8 call (the uint8 image between the passes; none when a pass is skipped)."""
    if in_h == out_h or in_w == out_w:
        return 0
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_RESAMPLE, n, in_h, out_w, 0, 0, 0))


def resample(ctx, src: int, in_h: int, in_w: int, in_pitch: int, dst: int, out_h: int, out_w: int, full_h: int, full_w: int, out_pitch: int,
             flt: int, n: int = 1) -> None:
    """ir_resample_u8 on the current stream; src / dst are device addresses. The scratch is the context's workspace (stream-ordered like
    every other call that uses it; a caller that has handed its address to a later launch grows it first, see chain_ws_bytes)."""
    plan = Plans.of(ctx).get(in_h, in_w, out_h, out_w, flt)
    need = ws_bytes(n, in_h, in_w, out_h, out_w)
    ws = ctx.workspace(need) if need else None
    ctx.check(ctx.lib.ir_resample_u8(ctx.h, ctx.stream(), C.c_void_p(src), n, in_h, in_w, in_pitch, C.c_void_p(dst), out_h, out_w, full_h, full_w,
                                     out_pitch, L.ptr(plan), L.ptr(ws), ws.numel() if need else 0), "ir_resample_u8")


def window_ws_bytes(n: int, in_h: int, in_w: int, out_h: int, out_w: int, win_w: int) -> int:
    """Workspace of one ir_resample_u8_window call: the intermediate holds win_w columns."""
    if in_h == out_h or in_w == out_w:
        return 0
    return int(L.load_library().ir_workspace_bytes(None, L.STAGE_RESAMPLE, n, in_h, win_w, 0, 0, 0))


def resample_window(ctx, src: int, in_h: int, in_w: int, in_pitch: int, dst: int, out_h: int, out_w: int, y0: int, x0: int, win_h: int, win_w: int,
                    full_h: int, full_w: int, out_pitch: int, flt: int, n: int = 1) -> None:
    """ir_resample_u8_window on the current stream: the window of the virtual out_h x out_w result into the top-left corner of dst."""
    plan = Plans.of(ctx).get(in_h, in_w, out_h, out_w, flt)
    need = window_ws_bytes(n, in_h, in_w, out_h, out_w, win_w)
    ws = ctx.workspace(need) if need else None
    ctx.check(ctx.lib.ir_resample_u8_window(ctx.h, ctx.stream(), C.c_void_p(src), n, in_h, in_w, in_pitch, C.c_void_p(dst), out_h, out_w, y0, x0, win_h,
                                            win_w, full_h, full_w, out_pitch, L.ptr(plan), L.ptr(ws), ws.numel() if need else 0), "ir_resample_u8_window")


def _crop_steps(rec: ResizeJob):
    """[(in_h, in_w, out_h, out_w, filter)] of the calls that take rec.raw to the size the centre crop's window is cut from. A step of equal
    size is left out (Pillow's resize to the same size copies) - but for the last one, which is the window call whatever its sizes."""
    sizes = [tuple(rec.raw.shape[:2])] + [(th, tw) for tw, th in rec.geo.chain]
    flts = rec.geo.filters or (BICUBIC,) * len(rec.geo.chain)
    steps, at = [], sizes[0]
    for k, (to, flt) in enumerate(zip(sizes[1:], flts)):
        if to != at or k + 2 == len(sizes):
            steps.append(at + to + (flt,))
        at = to
    return steps


def _steps(rec: ResizeJob):
    """[(in_h, in_w, out_h, out_w)] of the bicubic calls that take rec.raw to the network input (equal sizes: the padded copy); of a centre
    crop, the calls of _crop_steps()."""
    if rec.geo.crop is not None:
        return [s[:4] for s in _crop_steps(rec)]
    h, w = rec.raw.shape[:2]
    sizes = [(h, w)] + [(th, tw) for tw, th in rec.geo.chain]
    if len(sizes) == 1:
        sizes.append((h, w))
    return [a + b for a, b in zip(sizes[:-1], sizes[1:])]


def chain_ws_bytes(records: Sequence[ResizeJob]) -> int:
    """The largest workspace any resampling call of this batch needs, ahead of and behind the network."""
    need = 0
    for rec in records:
        steps = _steps(rec)
        if rec.geo.crop is not None:   # the last call makes the window's columns alone
            need = max(need, window_ws_bytes(1, *steps[-1], rec.geo.valid_hw[1]))
            steps = steps[:-1]
        for ih, iw, oh, ow in steps:
            need = max(need, ws_bytes(1, ih, iw, oh, ow))
        if rec.geo.lanczos:
            need = max(need, ws_bytes(1, *rec.geo.valid_hw, rec.geo.lanczos[1], rec.geo.lanczos[0]))
    return need


def _is_jpeg(raw) -> bool:
    from .jpeg_decode import JpegSource
    return isinstance(raw, JpegSource)


def _is_png(raw) -> bool:
    from .png_decode import PngSource
    return isinstance(raw, PngSource)


def _is_source(raw) -> bool:
    """A file the device decodes: its compressed bytes travel, and its image's place in d_raw is filled by decode()."""
    return _is_jpeg(raw) or _is_png(raw)


def decode_ws_bytes(records: Sequence[ResizeJob]) -> int:
    """Workspace of the batch's ir_jpeg_decode and ir_png_decode calls (the larger; 0 without such files)."""
    from . import jpeg_decode as J
    from . import png_decode as P
    jpegs = [rec.raw for rec in records if _is_jpeg(rec.raw)]
    pngs = [rec.raw for rec in records if _is_png(rec.raw)]
    return max(J.ws_bytes(jpegs) if jpegs else 0, P.ws_bytes(pngs) if pngs else 0)


def check_records(records: Sequence[ResizeJob]) -> Tuple[int, int, int]:
    if len(records) == 0:
        raise ValueError("resize: empty batch")
    for rec in records:
        a = rec.raw
        if not _is_source(a) and (not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3):
            raise ValueError("resize: the decoded files must be HWC uint8 RGB arrays (or jpeg_decode.JpegSource / png_decode.PngSource files)")
        if rec.geo.net_hw != records[0].geo.net_hw:
            raise ValueError("resize: the images of a batch must reach one network input size")
        last = rec.geo.chain[-1] if rec.geo.chain else (a.shape[1], a.shape[0])
        if rec.geo.crop is not None:   # a centre crop: the window lies in the chain's last size and is the network input as it is
            (top, left), (vh, vw) = rec.geo.crop, rec.geo.valid_hw
            if (not rec.geo.chain or len(rec.geo.filters or rec.geo.chain) != len(rec.geo.chain) or rec.geo.lanczos or tuple(rec.geo.net_hw) != (vh, vw)
                    or top < 0 or left < 0 or top + vh > last[1] or left + vw > last[0]):
                raise ValueError("resize: the crop geometry does not hold its window")
            continue
        if (last[1], last[0]) != tuple(rec.geo.valid_hw):
            raise ValueError("resize: the geometry does not belong to the decoded file")
    return (len(records),) + tuple(records[0].geo.net_hw)


def _lq_shape(rec: ResizeJob) -> tuple:
    """The shape of what ir_degrade reads and writes for a record: the decoded file, or the centre crop made of it."""
    return tuple(rec.geo.valid_hw) + (3,) if rec.geo.crop is not None else tuple(rec.raw.shape)


def _grown(t: Optional[torch.Tensor], nbytes: int, device=None, pinned=False) -> torch.Tensor:
    if t is not None and t.numel() >= nbytes:
        return t
    nbytes = max(int(nbytes * 1.25), 1 << 16)   # decoded files of one folder differ a little: do not re-allocate for every new maximum
    return torch.empty(nbytes, dtype=torch.uint8).pin_memory() if pinned else torch.empty(nbytes, dtype=torch.uint8, device=device)


class ResizeSlot(Pooled):
    """Buffers of one staging slot for batches whose images are resized on the device. Decoded files differ in size, so they get a flat
    page-locked buffer and its device copy (each file at a 256-byte boundary) instead of _Staging's fixed shape; `mid` holds the image
    between two chained calls (a pair used alternately: a centre crop's chain may be longer than two); d_crop holds the centre crops that
    ir_degrade reads; d_res / h_res hold the LANCZOS results (predictions, then stage-1 images) that are downloaded or
    encoded in place of the network's output. All grow on demand and are reused by the next batch of the slot."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.h_raw = self.d_raw = self.d_res = self.h_res = self.d_lq = self.h_lq = self.d_crop = None
        self.mid = [None, None]
        self.h2d_done = None
        self.fresh = False
        self.offsets: List[int] = []
        self.dparams = None      # degrade.Params of the batch in the slot, one per image, or None
        self.extras: List[tuple] = []   # per image the offsets of its blur kernel and noise field (or None) in h_raw / d_raw
        self.img_bytes = 0       # where the images end in h_raw / d_raw (the kernels and noise fields follow)
        self.lq_made = False
        self.lq_offsets: List[int] = []   # where every image's LQ image (and the centre crop it is made from) lies in d_lq / d_crop
        self.lq_bytes = 0
        self.jpeg: List[tuple] = []     # per JPEG file of the batch (a JpegSource record): its index and the offset of its compressed bytes
        self.png: List[tuple] = []      # the same per PNG file (a PngSource record)
        self.d_info = self.h_info = None   # ir_jpeg_decode's, then ir_png_decode's info words of the batch, device and page-locked

    def fill(self, records: Sequence[ResizeJob], degrade=None) -> None:
        """Copy the decoded files into the page-locked buffer (after the previous upload out of it has completed). degrade: one degrade.Params
        (or one degrade.ChainParams: a batch holds one kind) per image, or None - their blur kernels and noise fields travel behind the images.
        A JpegSource or PngSource keeps its image's place free and travels as compressed bytes behind all of that; decode() fills the place on
        the device."""
        if degrade is not None:
            from . import degrade as D
            if len(degrade) != len(records):
                raise ValueError("degrade: one parameter record per image")
            if len({isinstance(p, D.ChainParams) for p in degrade}) > 1:
                raise ValueError("degrade: a batch holds one kind of record (degrade.Params or degrade.ChainParams)")
            for rec, p in zip(records, degrade):
                D.check_params(p, *_lq_shape(rec)[:2])
        if self.h2d_done is not None:
            self.h2d_done.synchronize()
            self.h2d_done = None
        self.offsets, at = [], 0
        for rec in records:
            self.offsets.append(at)
            at += (rec.raw.size + 255) & ~255
        self.img_bytes, self.dparams, self.extras, self.lq_made = at, degrade, [], False
        self.lq_offsets, self.lq_bytes = [], 0
        for rec in records:   # the files' own offsets, but for centre crops: a crop may be larger than its file
            self.lq_offsets.append(self.lq_bytes)
            self.lq_bytes += (int(np.prod(_lq_shape(rec))) + 255) & ~255
        if degrade is not None:
            at += sum(D.extra_bytes(p) for p in degrade)
        self.jpeg, self.png = [], []
        for i, rec in enumerate(records):
            if _is_source(rec.raw):
                at = (at + 255) & ~255
                (self.jpeg if _is_jpeg(rec.raw) else self.png).append((i, at))
                at += rec.raw.blob_bytes
        self.h_raw = _grown(self.h_raw, at, pinned=True)
        if self.d_raw is None or self.d_raw.numel() < self.h_raw.numel():
            self.d_raw, self.fresh = _grown(None, self.h_raw.numel(), self.ctx.device), True
        self.used = at
        host = self.h_raw.numpy()
        for rec, o in zip(records, self.offsets):
            if not _is_source(rec.raw):
                np.copyto(host[o:o + rec.raw.size].reshape(rec.raw.shape), rec.raw)
        at = self.img_bytes
        for p in degrade or ():
            k_at, n_at, at = D.pack_extras(p, host, at)
            self.extras.append((k_at, n_at))
        for i, b_at in self.jpeg + self.png:
            records[i].raw.pack(host, b_at)

    def upload(self, stream=None, owner=None):
        """Asynchronous H2D copy of the decoded bytes on `stream` (default: the current one); the event behind it is what the next fill() waits for.
        owner: the stream the buffers are allocated and read on, when it is another one - a device buffer that has just been (re-)allocated may be
        memory that work queued on `owner` still uses, so the first copy into it waits for that stream."""
        if self.fresh and owner is not None and stream is not None:
            stream.wait_stream(owner)
        self.fresh = False
        first = self.img_bytes if len(self.jpeg) + len(self.png) == len(self.offsets) else 0   # a batch of compressed files alone uploads no pixels
        self.d_raw[first:self.used].copy_(self.h_raw[first:self.used], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream if stream is not None else torch.cuda.current_stream(self.ctx.device))
        self.h2d_done = ev
        return ev

    def decode(self, records: Sequence[ResizeJob]) -> None:
        """Between upload() and degrade() / to_network(), on the current stream: every JPEG file of the batch is decoded (ir_jpeg_decode, one call)
        and every PNG file (ir_png_decode, one call) into its image's place in d_raw. The info words - the JPEG files', then the PNG files' -
        follow with download_info() and are read by check_info()."""
        from . import jpeg_decode as J
        from . import png_decode as P
        n = len(self.jpeg) + len(self.png)
        if not n:
            return
        if self.d_info is None or self.d_info.numel() < n:
            self.d_info = torch.zeros(max(n, 16), dtype=torch.int32, device=self.ctx.device)
            self.h_info = torch.zeros(max(n, 16), dtype=torch.int32).pin_memory()
        base = self.d_raw.data_ptr()
        if self.jpeg:
            J.launch(self.ctx, [records[i].raw.record(base + b_at, base + self.offsets[i]) for i, b_at in self.jpeg], self.d_info.data_ptr())
        if self.png:
            P.launch(self.ctx, [records[i].raw.record(base + b_at, base + self.offsets[i]) for i, b_at in self.png],
                     self.d_info.data_ptr() + 4 * len(self.jpeg))

    def download_info(self) -> None:
        """Asynchronous D2H copy of decode()'s info words, on the current stream."""
        if self.jpeg or self.png:
            self.h_info.copy_(self.d_info, non_blocking=True)

    def check_info(self, records: Sequence[ResizeJob]) -> None:
        """After the copy has completed: a file the device could not decode ends the batch with an error that names it."""
        from . import jpeg_decode as J
        for k, (i, _) in enumerate(self.jpeg):
            cls = int(self.h_info[k])
            if cls:
                name = getattr(records[i].raw, "name", None) or f"image {i} of the batch"
                raise RuntimeError(f"ir_jpeg_decode: {name} is not a valid baseline JPEG stream ({J.ERRORS.get(cls, cls)})")
        from . import png_decode as P
        for k, (i, _) in enumerate(self.png):
            cls = int(self.h_info[len(self.jpeg) + k])
            if cls:
                name = getattr(records[i].raw, "name", None) or f"image {i} of the batch"
                raise RuntimeError(f"ir_png_decode: {name} is not a valid PNG stream ({P.ERRORS.get(cls, cls)})")

    def degrade(self, records: Sequence[ResizeJob]) -> None:
        """Between upload() and to_network(), on the current stream: every decoded file (ground truth) becomes its LQ image in d_lq, at the
        file's offset, by ir_degrade (ir_degrade_chain for ChainParams) with the parameters fill() staged. The files differ in size, so each is a call of its own.
        A centre crop is cut first, into d_crop, and the crop is what is degraded."""
        from . import degrade as D
        self.d_lq = _grown(self.d_lq, self.lq_bytes, self.ctx.device)
        if any(rec.geo.crop is not None for rec in records):
            self.d_crop = _grown(self.d_crop, self.lq_bytes, self.ctx.device)
        base = self.d_raw.data_ptr()
        for rec, p, o, lo, (k_at, n_at) in zip(records, self.dparams, self.offsets, self.lq_offsets, self.extras):
            h, w = _lq_shape(rec)[:2]
            src = base + o
            if rec.geo.crop is not None:
                src = self.d_crop.data_ptr() + lo
                self._crop(rec, base + o, src, h, w)
            if isinstance(p, D.ChainParams):   # k_at: the offsets of the chain's kernels and fields
                D.launch_chain_params(self.ctx, p, src, self.d_lq.data_ptr() + lo, h, w, base, k_at)
                continue
            D.launch(self.ctx, src, self.d_lq.data_ptr() + lo, h, 3 * w, h, w, [D.record(p, base + k_at, base + n_at if n_at is not None else None)])
        self.lq_made = True

    def download_lq(self) -> None:
        """Asynchronous D2H copy of the LQ images degrade() made, on the current stream."""
        self.h_lq = _grown(self.h_lq, self.lq_bytes, pinned=True)
        self.h_lq[:self.lq_bytes].copy_(self.d_lq[:self.lq_bytes], non_blocking=True)

    def host_lq(self, records: Sequence[ResizeJob]) -> List[np.ndarray]:
        """The downloaded LQ images (after the copy has completed) as arrays the caller owns."""
        host = self.h_lq.numpy()
        return [host[o:o + int(np.prod(_lq_shape(rec)))].reshape(_lq_shape(rec)).copy() for rec, o in zip(records, self.lq_offsets)]

    def to_network(self, records: Sequence[ResizeJob], d_in: torch.Tensor) -> None:
        """Per image the bicubic chain from its decoded bytes (its LQ image after degrade()) into its slot of d_in [n][h][w][3], zero padding
        included, on the current stream. A centre crop runs its chain (_crop): the last call writes the window alone, straight into d_in."""
        n, h, w, _ = d_in.shape
        for i, rec in enumerate(records):
            if rec.geo.crop is not None:
                if self.lq_made:   # the degraded crop is the network input as it is
                    vh, vw = rec.geo.valid_hw
                    resample(self.ctx, self.d_lq.data_ptr() + self.lq_offsets[i], vh, vw, 3 * vw, d_in[i].data_ptr(), vh, vw, h, w, 3 * w, BICUBIC)
                else:
                    self._crop(rec, self.d_raw.data_ptr() + self.offsets[i], d_in[i].data_ptr(), h, w)
                continue
            steps = _steps(rec)
            # the LQ images have offsets of their own: they differ from the files' as soon as a centre crop shares the batch
            src = self.d_lq.data_ptr() + self.lq_offsets[i] if self.lq_made else self.d_raw.data_ptr() + self.offsets[i]
            pitch = 3 * rec.raw.shape[1]
            for k, (ih, iw, oh, ow) in enumerate(steps):
                if k + 1 < len(steps):   # the uint8 image between two resizes, as the reference has one
                    self.mid[0] = _grown(self.mid[0], oh * ow * 3, self.ctx.device)
                    resample(self.ctx, src, ih, iw, pitch, self.mid[0].data_ptr(), oh, ow, oh, ow, 3 * ow, BICUBIC)
                    src, pitch = self.mid[0].data_ptr(), 3 * ow
                else:
                    resample(self.ctx, src, ih, iw, pitch, d_in[i].data_ptr(), oh, ow, h, w, 3 * w, BICUBIC)

    def _crop(self, rec: ResizeJob, src: int, dst: int, full_h: int, full_w: int) -> None:
        """The chain of a centre crop from the decoded file at src: the optional --sr_scale bicubic, the BOX halvings and the final bicubic,
        uint8 images between them as Pillow has them; the last call cuts the window into the top-left corner of dst [full_h][full_w][3]."""
        steps = _crop_steps(rec)
        (top, left), (vh, vw), pitch = rec.geo.crop, rec.geo.valid_hw, 3 * rec.raw.shape[1]
        for k, (ih, iw, oh, ow, flt) in enumerate(steps):
            if k + 1 < len(steps):
                mid = self.mid[k & 1] = _grown(self.mid[k & 1], oh * ow * 3, self.ctx.device)
                resample(self.ctx, src, ih, iw, pitch, mid.data_ptr(), oh, ow, oh, ow, 3 * ow, flt)
                src, pitch = mid.data_ptr(), 3 * ow
            else:
                resample_window(self.ctx, src, ih, iw, pitch, dst, oh, ow, top, left, vh, vw, full_h, full_w, 3 * full_w, flt)

    def reserve_results(self, n: int, h: int, w: int, with_stage1: bool) -> None:
        """Room for every image's result at up to the network's size (a LANCZOS target never exceeds it), before anything is queued."""
        need = (2 if with_stage1 else 1) * n * h * w * 3
        self.d_res = _grown(self.d_res, need, self.ctx.device)
        self.h_res = _grown(self.h_res, self.d_res.numel(), pinned=True)

    def back_to_lq(self, records: Sequence[ResizeJob], d_out: torch.Tensor, first: int) -> List[Optional[torch.Tensor]]:
        """Behind the network, on the current stream: the valid rectangle of every image of d_out [n][h][w][3] that names a LANCZOS target is
        resampled into result slot first + i. Returns per image its result as a device tensor [1][th][tw][3], or None (a plain crop)."""
        n, h, w, _ = d_out.shape
        res = []
        for i, rec in enumerate(records):
            if not rec.geo.lanczos:
                res.append(None)
                continue
            (tw, th), (vh, vw) = rec.geo.lanczos, rec.geo.valid_hw
            o = (first + i) * h * w * 3
            dst = self.d_res[o:o + th * tw * 3]
            resample(self.ctx, d_out[i].data_ptr(), vh, vw, 3 * w, dst.data_ptr(), th, tw, th, tw, 3 * tw, LANCZOS)
            res.append(dst.view(1, th, tw, 3))
        return res

    def download(self, results: Sequence[Optional[torch.Tensor]]) -> None:
        """Asynchronous D2H copies of the given results (views of d_res) into the same places of h_res, on the current stream."""
        base = self.d_res.data_ptr()
        for r in results:
            if r is not None:
                o = r.data_ptr() - base
                self.h_res[o:o + r.numel()].copy_(self.d_res[o:o + r.numel()], non_blocking=True)

    def host_result(self, r: torch.Tensor) -> np.ndarray:
        """The downloaded result (after the copy has completed) as an array the caller owns."""
        o = r.data_ptr() - self.d_res.data_ptr()
        return self.h_res[o:o + r.numel()].numpy().reshape(tuple(r.shape[1:])).copy()
