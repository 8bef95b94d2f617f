"""PNG files from the device encoder (ir_png_encode, csrc/png_encode.hip): the GPU produces the zlib stream of the Paeth-filtered rows,
the host adds the chunk framing - signature, IHDR, IDAT with its CRC, IEND - which costs one CRC-32 over the compressed bytes instead
of a deflate over the pixels.

The encoder codes literals only (one dynamic-Huffman block per 8 rows, no LZ77 matches), so a byte never costs less than one bit: on
restored photographs its files are 10 - 18 % smaller than zlib level 1's and within a few percent of PIL's default level, on flat or
near-flat content (smooth sky, graphics) they are several times larger than PIL's. It is an encoder for photographs, and opt-in.

The run mode (ir_png_encode_runs, PngEncoder(runs=True), --png_runs) lifts that limit and is opt-in as well; the default mode is unchanged. Per
chunk of 8 rows it also prices a block in which every run of equal filtered bytes is one literal and matches at distance 1 (pieces of 258 bytes,
a remainder of at least 6 as one more match) with a compacted header (zero-repeat symbols in the code-length section), and writes the cheaper of
the two blocks: the same pixels, no stream longer than the default mode's, ir_png_bound and the buffers below as they are. Stream bytes of
the format's CPU model (tests/support/png_runs_model.py) on 512 x 512 cases, measured on the CPU; the device's streams have the model's
lengths (tests/test_png_runs_gpu.py):
                     default mode   run mode   PIL level 1   PIL level 6 (files)
    constant              107 587      3 014         4 408         1 879
    smooth sky            109 748     17 402        16 212         9 422
    12 flat regions       110 075      9 785        10 132         5 685
    sky over photograph   221 930    172 141       208 982       175 239
    grainy photograph     332 194    324 948       395 270       335 220
Measured on one MI355X (profiles/png_runs.txt): 0.72 ms per 2048 x 2048 result against the default mode's 0.38 ms, 0.61 % of the step.
"""
import ctypes as C
import struct
import zlib
from typing import List, Sequence, Tuple

import torch

from . import _lib as L

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
IDAT_LIMIT = 1 << 30   # a chunk's length field holds 2^31 - 1; streams beyond this are split over several IDATs


def _chunk(kind: bytes, data) -> List[bytes]:
    crc = zlib.crc32(data, zlib.crc32(kind))
    return [struct.pack(">I", len(data)), kind, data, struct.pack(">I", crc)]


def wrap_png(zlib_stream, width: int, height: int) -> bytes:
    """The PNG file (8-bit RGB, non-interlaced, no ancillary chunks - what PIL writes for mode RGB) around a zlib stream of its filtered scanlines."""
    if width < 1 or height < 1:
        raise ValueError("wrap_png: empty image")
    view = memoryview(zlib_stream)
    parts = [_SIGNATURE] + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
    for o in range(0, max(len(view), 1), IDAT_LIMIT):
        parts += _chunk(b"IDAT", view[o:o + IDAT_LIMIT])
    return b"".join(parts + _chunk(b"IEND", b""))


def bound(h: int, w: int) -> int:
    """ir_png_bound: bytes that hold the stream of any h x w image."""
    return int(L.load_library().ir_png_bound(h, w))


class PngEncoder:
    """Device and page-locked host buffers for the streams of up to `count` images of at most h x w pixels, and the calls around them:
    queue() puts ir_png_encode for a batch on the current stream, fetch_sizes() / fetch() bring back the byte counts and then only the
    bytes produced. One instance per batch shape and staging slot (pipeline.process_stream keeps them on the context). runs: queue() calls
    ir_png_encode_runs, the run mode, with that stage's workspace; everything else is the same."""

    def __init__(self, ctx, count: int, h: int, w: int, runs: bool = False):
        self.ctx, self.count, self.h, self.w, self.runs = ctx, count, h, w, bool(runs)
        self.stride = (bound(h, w) + 255) & ~255
        self.d_out = torch.empty((count, self.stride), dtype=torch.uint8, device=ctx.device)
        self.d_info = torch.zeros(count, dtype=torch.int32, device=ctx.device)
        self.h_out = torch.empty((count, self.stride), dtype=torch.uint8).pin_memory()
        self.h_info = torch.zeros(count, dtype=torch.int32).pin_memory()
        self.rects: List[Tuple[int, int]] = [(h, w)] * count

    def queue(self, first: int, images: torch.Tensor, rects: Sequence[Tuple[int, int]]) -> None:
        """Encode the valid rectangles rects[i] = (vh, vw) of images [n][h][w][3] (device uint8) into slots first .. first + n - 1, on the current
        stream. Images of one rectangle share a call; the scratch is the context's workspace (the calls are stream-ordered)."""
        n, h, w, _ = images.shape
        if len(rects) != n or first + n > self.count or h > self.h or w > self.w:
            raise ValueError("PngEncoder.queue: batch does not fit the buffers")
        ctx = self.ctx
        i = 0
        while i < n:
            k = i + 1
            while k < n and tuple(rects[k]) == tuple(rects[i]):
                k += 1
            vh, vw = (int(v) for v in rects[i])
            ws = ctx.workspace(ctx.ws_bytes(L.STAGE_PNG_RUNS if self.runs else L.STAGE_PNG, k - i, vh, vw))
            name = "ir_png_encode_runs" if self.runs else "ir_png_encode"
            ctx.check(getattr(ctx.lib, name)(ctx.h, ctx.stream(), C.c_void_p(images[i].data_ptr()), k - i, h, w, 3 * w, vh, vw,
                                             C.c_void_p(self.d_out[first + i].data_ptr()), self.stride, C.c_void_p(self.d_info[first + i].data_ptr()),
                                             L.ptr(ws), ws.numel()), name)
            for j in range(i, k):
                self.rects[first + j] = (vh, vw)
            i = k

    def fetch_sizes(self) -> None:
        """Asynchronous download of the byte counts on the current stream."""
        self.h_info.copy_(self.d_info, non_blocking=True)

    def fetch(self, used: int, stream=None, wrap: bool = True) -> list:
        """After fetch_sizes() has completed: download the produced bytes of slots 0 .. used - 1 on `stream` (default: the current one), wait, and
        return the PNG files - or, with wrap=False, (zlib stream, width, height) triples for a later wrap_png(*triple) on another thread (the CRC-32
        and the copies of a 2048 x 2048 result cost about 20 ms, which the caller's thread then does not pay)."""
        stream = stream or torch.cuda.current_stream(self.ctx.device)
        sizes = [int(v) for v in self.h_info[:used].tolist()]
        with torch.cuda.stream(stream):
            for i, size in enumerate(sizes):
                if not 6 < size <= self.stride:
                    raise RuntimeError(f"ir_png_encode reported {size} bytes for a slot of {self.stride}")
                self.h_out[i, :size].copy_(self.d_out[i, :size], non_blocking=True)
        stream.synchronize()
        host = self.h_out.numpy()
        if not wrap:
            return [(host[i, :size].tobytes(), self.rects[i][1], self.rects[i][0]) for i, size in enumerate(sizes)]
        return [wrap_png(host[i, :size], self.rects[i][1], self.rects[i][0]) for i, size in enumerate(sizes)]
