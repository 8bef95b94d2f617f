"""PNG inputs for the device decoder (ir_png_decode, csrc/png_decode.hip): the host walks the chunks - IHDR, a CRC-32 per chunk as Pillow checks
it, the IDAT payloads joined into one zlib stream - and inflates nothing; the GPU finds the deflate blocks, decodes them in parallel, follows the
copies, checks the Adler-32, unfilters and converts to RGB. The pixels are Pillow's, np.array(Image.open(f).convert("RGB")), byte for byte;
tools/png_decode_model.py is the definition both are tested against.

PngSource.open() takes what the kernels take - 8 bits a sample, colour type 0 / 2 / 4 / 6, not interlaced - and refuses everything else with a
one-word reason, so that the caller falls back to Pillow for exactly those files. A PngSource stands where resample.ResizeJob.raw holds a decoded
array: it has the array's .shape and .size, and its compressed bytes are staged instead of the pixels.
"""
import ctypes as C
import struct
import zlib
from typing import NamedTuple, Optional, Sequence

import numpy as np

SPAN_BITS = 65536     # the one value the product uses: 14.4 ms per 2048 x 2048 file against 14.9 / 14.8 / 29.6 / 72.4 ms at 4096 / 16384 / 2^18 / 2^20 (profiles/png_decoder.txt)
SPAN_MIN, SPAN_MAX = 256, 1 << 20
FIXED_LIMIT = 65536   # a longer stream that begins with a fixed-Huffman block is refused: no header the finder could recognise
UNFILTER_LANES = 1024   # IR_PNG_UNFILTER_LANES: rows the unfilter workgroup takes at a time
ADLER_CHUNK = 16384     # IR_PNG_ADLER_CHUNK
ERRORS = {1: "bad block type or header", 2: "invalid code", 3: "read past the end", 4: "distance before the start", 5: "stored-length mismatch",
          6: "wrong inflated size", 7: "Adler-32 mismatch", 8: "filter type above 4"}
BPP = {0: 1, 2: 3, 4: 2, 6: 4}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
NONE = 0xffffffff


def _up4(v: int) -> int:
    return (v + 3) & ~3


def _up256(v: int) -> int:
    return (v + 255) & ~255


class Layout(NamedTuple):
    """The workspace's sections (include/instarevive_hip.h), byte offsets: ir_png_decode_layout in Python, for the tests and tools that read them."""
    spans: int
    entries: int
    cap: int
    chunks: int
    hdr: int
    cand: int
    e_end: int
    e_next: int
    e_len: int
    e_status: int
    e_off: int
    chain: int
    adler: int
    src: int
    lit: int
    bytes: int
    pix: int
    total: int


def layout(h: int, w: int, stream_bytes: int, span_bits: int) -> Layout:
    spans = -(-stream_bytes * 8 // span_bits)
    entries, cap = spans + 1, h * (1 + 4 * w)
    chunks = -(-cap // ADLER_CHUNK)
    at, offs = 0, []
    for nbytes in (256, 4 * spans) + (4 * entries,) * 6 + (8 * chunks, 4 * cap, cap, cap + 32, h * (4 * w + 32)):
        offs.append(at)
        at += _up256(nbytes)
    return Layout(spans, entries, cap, chunks, *offs, at)


class PngSource:
    """A PNG file ready for ir_png_decode: the header's numbers and the zlib stream, zero-padded to a multiple of 4 bytes. Stands where
    ResizeJob.raw holds a decoded array: .shape is (h, w, 3) and .size the bytes of the decoded image. blob is what travels to the device."""

    def __init__(self, h: int, w: int, color_type: int, stream: np.ndarray, adler: int):
        self.h, self.w, self.color_type, self.adler = h, w, color_type, adler
        self.bpp = BPP[color_type]
        self.stream = stream   # uint8, a multiple of 4 bytes; its own: a test may damage it in place
        self.shape = (h, w, 3)
        self.size = h * w * 3
        self.ndim, self.dtype = 3, np.dtype(np.uint8)
        self.inflated = h * (1 + w * self.bpp)
        self.name = None

    @property
    def blob_bytes(self) -> int:
        return self.stream.size

    @staticmethod
    def open(data: bytes):
        """-> (PngSource, None) or (None, reason): one pass over the chunks, nothing inflated."""
        data = bytes(data)
        if len(data) < 8 or data[:8] != SIGNATURE:
            return None, "format"
        at, n, ihdr, parts, ended = 8, len(data), None, [], False
        while at < n:
            if at + 12 > n:
                return None, "truncated"
            size, kind = struct.unpack_from(">I4s", data, at)
            if at + 12 + size > n:
                return None, "truncated"
            body = data[at + 8:at + 8 + size]
            if zlib.crc32(data[at + 4:at + 8 + size]) != struct.unpack_from(">I", data, at + 8 + size)[0]:
                return None, "crc"
            at += 12 + size
            if ihdr is None:
                if kind != b"IHDR" or size != 13:
                    return None, "format"
                ihdr = struct.unpack(">IIBBBBB", body)
            elif kind == b"IDAT":
                parts.append(body)
            elif kind == b"tRNS":
                return None, "transparency"
            elif kind == b"acTL":
                return None, "animated"
            elif kind == b"IEND":
                ended = True
                break
        if ihdr is None or not ended:
            return None, "truncated"
        w, h, depth, color_type, comp, flt, interlace = ihdr
        if color_type == 3:
            return None, "palette"
        if color_type not in BPP or comp != 0 or flt != 0:
            return None, "format"
        if depth != 8:
            return None, "depth"
        if interlace:
            return None, "interlaced"
        if not (1 <= w <= 65535 and 1 <= h <= 65535) or h * (1 + 4 * w) >= 1 << 31:
            return None, "size"
        z = b"".join(parts)
        if len(z) < 6:
            return None, "short"
        if len(z) + 8 > 1 << 28:
            return None, "size"
        if (z[0] & 15) != 8 or (z[0] >> 4) > 7 or (z[1] & 0x20) or ((z[0] << 8) | z[1]) % 31:
            return None, "zlib"
        if len(z) > FIXED_LIMIT and ((z[2] >> 1) & 3) == 1:
            return None, "fixed"
        stream = np.zeros(max(_up4(len(z)), 8), dtype=np.uint8)
        stream[:len(z)] = np.frombuffer(z, dtype=np.uint8)
        return PngSource(h, w, color_type, stream, struct.unpack(">I", z[-4:])[0]), None

    def pack(self, host: np.ndarray, at: int) -> None:
        """Copy the blob into the uint8 array `host` at byte `at` (a multiple of 4)."""
        host[at:at + self.stream.size] = self.stream

    def record(self, blob_addr: int, out_addr: int, pitch: Optional[int] = None):
        """The ir_png_file of this file with its blob at device address blob_addr and its image at out_addr."""
        from . import _lib as L
        return L.PngFile(blob_addr, out_addr, self.stream.size, self.adler, self.h, self.w, self.color_type, pitch if pitch is not None else 3 * self.w)


def ws_bytes(sources: Sequence[PngSource], span_bits: int = SPAN_BITS) -> int:
    """Workspace of one ir_png_decode call over these files (they share it)."""
    from . import _lib as L
    lib = L.load_library()
    return int(lib.ir_workspace_bytes(None, L.STAGE_PNG_DECODE, len(sources), max(s.h for s in sources), max(s.w for s in sources),
                                      max(s.stream.size for s in sources), span_bits, 0))


def launch(ctx, records: list, info_addr: int, span_bits: int = SPAN_BITS, ws=None) -> None:
    """ir_png_decode of the given ir_png_file records on the current stream; info_addr: device uint32 [n]. The scratch is the context's
    workspace unless ws (a device uint8 tensor) is given."""
    from . import _lib as L
    arr = (L.PngFile * len(records))(*records)
    if ws is None:
        need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_PNG_DECODE, len(records), max(r.h for r in records), max(r.w for r in records),
                                              max(r.stream_bytes for r in records), span_bits, 0))
        ws = ctx.workspace(need)
    ctx.check(ctx.lib.ir_png_decode(ctx.h, ctx.stream(), arr, len(records), span_bits, C.c_void_p(info_addr), L.ptr(ws), ws.numel()), "ir_png_decode")


def decode(ctx, sources: Sequence[PngSource], span_bits: int = SPAN_BITS, pitches: Optional[Sequence[int]] = None, fill: Optional[int] = None,
           want_ws: bool = False, guard: int = 0):
    """Decode files on the device, the plain way (tests, tools): -> (images as uint8 device tensors [h][pitch], info as a list, the workspace as a
    host uint8 array or None). fill: the byte the image buffers hold before the call. guard: bytes of `fill` kept in front of and behind every
    image and behind the workspace; they are checked after the call (AssertionError)."""
    import torch
    at, offs = 0, []
    for s in sources:
        offs.append(at)
        at += _up256(s.blob_bytes)
    host = torch.zeros(at, dtype=torch.uint8)
    for s, o in zip(sources, offs):
        s.pack(host.numpy(), o)
    dev = host.to(ctx.device)
    pitches = list(pitches) if pitches is not None else [3 * s.w for s in sources]
    fill = 0 if fill is None else fill
    bufs = [torch.full((s.h * p + 2 * guard,), fill, dtype=torch.uint8, device=ctx.device) for s, p in zip(sources, pitches)]
    outs = [b[guard:guard + s.h * p].view(s.h, p) for b, s, p in zip(bufs, sources, pitches)]
    info = torch.full((len(sources),), 0x7fffffff, dtype=torch.int32, device=ctx.device)
    need = ws_bytes(sources, span_bits)
    ws = torch.full((need + guard,), fill, dtype=torch.uint8, device=ctx.device)
    recs = [s.record(dev.data_ptr() + o, out.data_ptr(), p) for s, o, out, p in zip(sources, offs, outs, pitches)]
    launch(ctx, recs, info.data_ptr(), span_bits, ws=ws[:need])
    torch.cuda.synchronize(ctx.device)
    if guard:
        for b in bufs:
            assert bool((b[:guard] == fill).all()) and bool((b[-guard:] == fill).all()), "ir_png_decode wrote outside an image"
        assert bool((ws[need:] == fill).all()), "ir_png_decode wrote behind its workspace"
    return outs, [int(v) for v in info.tolist()], ws[:need].cpu().numpy() if want_ws else None


def tables(ws: np.ndarray, src: PngSource, span_bits: int, lay: Optional[Layout] = None) -> dict:
    """The last file's tables out of a workspace decode(..., want_ws=True) returned: what tools/png_decode_model.py states, under its names."""
    lay = lay or layout(src.h, src.w, src.stream.size, span_bits)
    u32 = lambda at, n: ws[at:at + 4 * n].view(np.uint32).copy()
    spans = -(-src.stream.size * 8 // span_bits)
    hdr = u32(lay.hdr, 64)
    n = src.inflated
    return dict(error=int(hdr[0]), chain=u32(lay.chain, spans + 1)[:int(hdr[1])], total=int(hdr[2]), adler=int(hdr[3]), cand=u32(lay.cand, spans),
                end=u32(lay.e_end, spans + 1), next=u32(lay.e_next, spans + 1), length=u32(lay.e_len, spans + 1), status=u32(lay.e_status, spans + 1),
                offset=u32(lay.e_off, spans + 1), flags=hdr[16:56], bytes=ws[lay.bytes:lay.bytes + n].copy(), src=u32(lay.src, n),
                lit=ws[lay.lit:lay.lit + n].copy())
