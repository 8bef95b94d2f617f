"""JPEG inputs for the device decoder (ir_jpeg_decode, csrc/jpeg_decode.hip): the host reads the markers and removes the byte stuffing - vectorised
numpy over the compressed bytes, no pixel loop - and the GPU does the rest: Huffman decode in parallel on the serial stream, DC prediction,
dequantisation, libjpeg's ISLOW inverse DCT, fancy upsampling, YCbCr -> RGB. The pixels are Pillow's, np.array(Image.open(f).convert("RGB")),
byte for byte; tools/jpeg_decode_model.py is the definition both are tested against.

parse() takes what the kernels take - baseline (SOF0), 8 bits, one interleaved scan, grey or YCbCr with luma 1x1 / 2x1 / 2x2 - and refuses
everything else with a one-word reason, so that the caller falls back to Pillow for exactly those files. A JpegSource stands where
resample.ResizeJob.raw holds a decoded array: it has the array's .shape and .size, and its compressed bytes are staged instead of the pixels.
"""
import ctypes as C
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

SUBSEQ_BITS = 1024   # the one value the product uses: 1.94 ms per 2048 x 2048 file against 26.1 / 4.87 / 2.82 ms at 256 / 512 / 2048 (profiles/jpeg_decoder.txt)
MIN_EDGE = 8         # below it libjpeg replicates chroma instead of interpolating it (a chroma row of two or fewer samples)
TABLE_BYTES = 6176   # IR_JPEG_DECODE_TABLE_BYTES
ERRORS = {1: "invalid Huffman code", 2: "coefficient index past 63", 3: "read past the restart interval's bits", 4: "wrong block count for a restart interval"}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Plan(NamedTuple):
    """What the headers say, in the decoder's terms. comps: 1 or 3; hs, vs: the luma sampling (1, 1 for one component); restart: MCUs per
    restart interval, 0 without DRI; tq / td / ta: per component the quantisation table and the DC and AC Huffman table; quant: {id: 64 values
    in natural order}; huff: {(class, id): (16 counts, symbols)}; scan: the bytes from behind the SOS header to the marker that ends the scan;
    segments: entropy_segments() of the scan as parse() made it (read-only), or None."""
    h: int
    w: int
    comps: int
    hs: int
    vs: int
    restart: int
    tq: tuple
    td: tuple
    ta: tuple
    quant: dict
    huff: dict
    scan: bytes
    segments: Optional[tuple] = None

    @property
    def mcu_grid(self) -> Tuple[int, int]:
        """(MCU rows, MCU columns)"""
        return -(-self.h // (8 * self.vs)), -(-self.w // (8 * self.hs))

    @property
    def blocks_per_mcu(self) -> int:
        return self.hs * self.vs + 2 if self.comps == 3 else 1

    @property
    def n_intervals(self) -> int:
        my, mx = self.mcu_grid
        return -(-my * mx // self.restart) if self.restart else 1

    def interval_mcus(self, j: int) -> int:
        my, mx = self.mcu_grid
        return min(self.restart, my * mx - j * self.restart) if self.restart else my * mx


_SOF_REASON = {0xC1: "extended", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "extended", 0xC6: "progressive", 0xC7: "lossless", 0xC9: "arithmetic", 0xCA: "arithmetic",
               0xCB: "arithmetic", 0xCD: "arithmetic", 0xCE: "arithmetic", 0xCF: "arithmetic"}


def parse(data: bytes):
    """-> (Plan, None), or (None, reason) for a file the device decoder does not take."""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        return None, "format"
    at, n = 2, len(data)
    quant, huff, frame, restart, jfif, adobe = {}, {}, None, 0, False, None
    while True:
        while at < n and data[at] != 0xFF:   # libjpeg skips to the next marker
            at += 1
        while at < n and data[at] == 0xFF:   # fill bytes
            at += 1
        if at + 2 >= n:
            return None, "truncated"
        marker, at = data[at], at + 1
        if marker == 0xD8 or 0xD0 <= marker <= 0xD7 or marker == 0x01:
            continue
        if marker == 0xD9:
            return None, "truncated"   # EOI in front of any scan
        size = struct.unpack_from(">H", data, at)[0]
        if size < 2 or at + size > n:
            return None, "truncated"
        seg, at = data[at + 2:at + size], at + size
        if marker == 0xC0:
            if frame is not None or len(seg) < 6:
                return None, "format"
            prec, h, w, nc = struct.unpack_from(">BHHB", seg)
            if prec != 8:
                return None, "precision"
            if len(seg) < 6 + 3 * nc:
                return None, "truncated"
            frame = (h, w, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)])
        elif marker in _SOF_REASON:
            if len(seg) >= 1 and seg[0] != 8 and marker == 0xC1:
                return None, "precision"
            return None, _SOF_REASON[marker]
        elif marker == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    return None, "quantisation"
                if p + 65 > len(seg) or (seg[p] & 15) > 3:
                    return None, "format"
                nat = np.zeros(64, dtype=np.uint16)
                nat[ZIGZAG] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=p + 1)
                quant[seg[p] & 15], p = nat, p + 65
        elif marker == 0xC4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    return None, "format"
                counts = list(seg[p + 1:p + 17])
                total = sum(counts)
                if (seg[p] >> 4) > 1 or (seg[p] & 15) > 1 or total > 256 or p + 17 + total > len(seg):
                    return None, "table" if (seg[p] & 15) > 1 else "format"
                code = 0
                for l, c in enumerate(counts, 1):   # more codes of a length than the prefix code has room for
                    code += c
                    if code > 1 << l:
                        return None, "format"
                    code <<= 1
                huff[(seg[p] >> 4, seg[p] & 15)] = (counts, list(seg[p + 17:p + 17 + total]))
                p += 17 + total
        elif marker == 0xDD:
            if len(seg) < 2:
                return None, "format"
            restart = struct.unpack_from(">H", seg)[0]
        elif marker == 0xDC:
            return None, "dnl"
        elif marker == 0xE0 and seg[:5] == b"JFIF\x00":
            jfif = True
        elif marker == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif marker == 0xDA:
            break
    if frame is None:
        return None, "format"
    h, w, comps = frame
    if len(comps) not in (1, 3):
        return None, "components"
    if h == 0:
        return None, "dnl"
    if len(comps) == 3 and not jfif:   # libjpeg's guess of the colour space (jdapimin.c:default_decompress_parms)
        ids = tuple(c[0] for c in comps)
        if (adobe is not None and adobe != 1) or (adobe is None and ids == (0x52, 0x47, 0x42)):
            return None, "colourspace"
    ns = seg[0] if seg else 0
    if ns != len(comps) or len(seg) < 1 + 2 * ns + 3:
        return None, "scans"
    if [seg[1 + 2 * i] for i in range(ns)] != [c[0] for c in comps] or tuple(seg[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
        return None, "scans"
    td, ta = tuple(seg[2 + 2 * i] >> 4 for i in range(ns)), tuple(seg[2 + 2 * i] & 15 for i in range(ns))
    tq = tuple(c[3] for c in comps)
    if len(comps) == 1:
        hs = vs = 1   # a single-component scan has 8 x 8 MCUs whatever its sampling factors say
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None, "sampling"
    if any(t not in quant for t in tq) or any((0, t) not in huff for t in td) or any((1, t) not in huff for t in ta):
        return None, "table"
    if h < MIN_EDGE or w < MIN_EDGE:
        return None, "small"
    # the scan ends at the first marker that is neither a stuffed zero, a fill byte nor RSTn
    a = np.frombuffer(data, dtype=np.uint8, offset=at)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    ends = ff[(nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))]
    if len(ends) == 0:
        return None, "truncated"
    end = int(ends[0])
    if a[end + 1] != 0xD9:
        return None, "dnl" if a[end + 1] == 0xDC else "scans"
    plan = Plan(h, w, len(comps), hs, vs, restart, tq, td, ta, quant, huff, data[at:at + end])
    segments = entropy_segments(plan)
    if segments is None:
        return None, "restart"
    for x in segments:
        x.setflags(write=False)
    return plan._replace(segments=segments), None


def entropy_segments(plan: Plan):
    """The scan's bytes with the stuffing, the fill bytes and the RSTn markers removed, every restart interval at a 4-byte boundary (zeros
    between, the whole a multiple of 4 bytes), and the table [intervals][2] uint32 of byte offsets and bit counts. None for a wrong RSTn number
    or a count of intervals that is not the headers'."""
    if plan.segments is not None:
        return plan.segments
    a = np.concatenate([np.frombuffer(plan.scan, dtype=np.uint8), np.array([0xFF], dtype=np.uint8)])   # + the first byte of the marker that ends the scan
    keep = np.ones(len(a), dtype=bool)
    keep[-1] = False
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    keep[ff[nxt == 0] + 1] = False      # the stuffed zero
    keep[ff[nxt == 0xFF]] = False       # a fill byte in front of a marker
    rst = ff[(nxt >= 0xD0) & (nxt <= 0xD7)]
    keep[rst], keep[rst + 1] = False, False
    if not np.array_equal(a[rst + 1] - 0xD0, np.arange(len(rst)) % 8) or len(rst) + 1 != plan.n_intervals:
        return None
    if len(rst) == 0:   # one interval: the kept bytes as they are
        kept = a[keep]
        stream = np.zeros(max(_up4(len(kept)), 4), dtype=np.uint8)
        stream[:len(kept)] = kept
        return stream, np.array([[0, 8 * len(kept)]], dtype=np.uint32)
    interval = np.zeros(len(a), dtype=np.int64)
    interval[rst] = 1
    interval = np.cumsum(interval)[keep]
    lengths = np.bincount(interval, minlength=len(rst) + 1)
    offsets = np.concatenate([[0], np.cumsum((lengths + 3) & ~3)])
    starts = np.concatenate([[0], np.cumsum(lengths)])
    stream = np.zeros(max(int(offsets[-1]), 4), dtype=np.uint8)
    stream[np.arange(len(interval)) - starts[interval] + offsets[interval]] = a[keep]
    table = np.stack([offsets[:-1], lengths * 8], axis=1).astype(np.uint32)
    return stream, table


def huffman_tables(spec):
    """One Huffman table (16 counts, symbols) in the kernel's form: the 9-bit first level, per length one past the last code left-aligned in 16
    bits, per length the symbol index of the first code minus that code, the symbols."""
    counts, vals = spec
    lut, limit, valoff = np.zeros(512, dtype=np.uint16), np.zeros(17, dtype=np.uint32), np.zeros(17, dtype=np.int32)
    sym = np.zeros(256, dtype=np.uint8)
    sym[:len(vals)] = vals
    code, k = 0, 0
    for l in range(1, 17):
        valoff[l] = k - code
        if l <= 9 and counts[l - 1]:
            span = 1 << (9 - l)
            first = code << (9 - l)
            lut[first:first + counts[l - 1] * span] = (l << 8) | np.repeat(np.asarray(vals[k:k + counts[l - 1]], dtype=np.uint16), span)
        code, k = code + counts[l - 1], k + counts[l - 1]
        limit[l] = code << (16 - l)
        code <<= 1
    return lut, limit, valoff, sym


def table_blob(plan: Plan) -> np.ndarray:
    """IR_JPEG_DECODE_TABLE_BYTES bytes: lut [4][512] u16, limit [4][17] u32, valoff [4][17] i32, vals [4][256] u8, quant [4][64] u16; the
    Huffman tables in the order DC 0, DC 1, AC 0, AC 1 (a table the file does not define stays zero: every code is invalid)."""
    lut, limit, valoff = np.zeros((4, 512), dtype=np.uint16), np.zeros((4, 17), dtype=np.uint32), np.zeros((4, 17), dtype=np.int32)
    vals, quant = np.zeros((4, 256), dtype=np.uint8), np.ones((4, 64), dtype=np.uint16)
    for (cls, tid), spec in plan.huff.items():
        lut[2 * cls + tid], limit[2 * cls + tid], valoff[2 * cls + tid], vals[2 * cls + tid] = huffman_tables(spec)
    for tid, q in plan.quant.items():
        quant[tid] = q
    blob = np.concatenate([x.view(np.uint8).reshape(-1) for x in (lut, limit, valoff, vals, quant)])
    assert blob.size == TABLE_BYTES
    return blob


def _up4(v: int) -> int:
    return (v + 3) & ~3


class JpegSource:
    """A JPEG file ready for ir_jpeg_decode: the plan, the unstuffed bytes, the interval table and the tables in the kernel's format. Stands where
    ResizeJob.raw holds a decoded array: .shape is (h, w, 3) and .size the bytes of the decoded image. blob is what travels to the device
    (stream | interval table | tables, each at a 4-byte boundary)."""

    def __init__(self, plan: Plan):
        self.plan = plan
        self.stream, self.intervals = (x.copy() for x in entropy_segments(plan))   # its own: a test may damage them in place
        self.tables = table_blob(plan)
        self.shape = (plan.h, plan.w, 3)
        self.size = plan.h * plan.w * 3
        self.ndim, self.dtype = 3, np.dtype(np.uint8)
        self.iv_at = _up4(self.stream.size)
        self.tab_at = self.iv_at + self.intervals.size * 4
        self.blob_bytes = self.tab_at + TABLE_BYTES

    @staticmethod
    def open(data: bytes):
        """-> (JpegSource, None) or (None, reason): parse() and the byte pass."""
        plan, why = parse(data)
        return (JpegSource(plan), None) if plan is not None else (None, why)

    def pack(self, host: np.ndarray, at: int) -> None:
        """Copy the blob into the uint8 array `host` at byte `at` (a multiple of 4)."""
        host[at:at + self.stream.size] = self.stream
        host[at + self.stream.size:at + self.iv_at] = 0
        host[at + self.iv_at:at + self.tab_at] = self.intervals.view(np.uint8).reshape(-1)
        host[at + self.tab_at:at + self.blob_bytes] = self.tables

    def record(self, blob_addr: int, out_addr: int, pitch: Optional[int] = None):
        """The ir_jpeg_file of this file with its blob at device address blob_addr and its image at out_addr."""
        from . import _lib as L
        p = self.plan
        pad = lambda t: (C.c_uint8 * 4)(*(tuple(t) + (0,) * 4)[:4])
        return L.JpegFile(blob_addr, blob_addr + self.iv_at, blob_addr + self.tab_at, out_addr, pitch if pitch is not None else 3 * p.w,
                          self.stream.size, len(self.intervals), p.h, p.w, p.comps, p.hs, p.vs, p.restart, pad(p.tq), pad(p.td), pad(p.ta))

    @property
    def blocks(self) -> int:
        my, mx = self.plan.mcu_grid
        return my * mx * self.plan.blocks_per_mcu


def ws_bytes(sources: Sequence[JpegSource], subseq_bits: int = SUBSEQ_BITS) -> int:
    """Workspace of one ir_jpeg_decode call over these files (they share it)."""
    from . import _lib as L
    lib = L.load_library()
    return int(lib.ir_workspace_bytes(None, L.STAGE_JPEG_DECODE, len(sources), max(s.plan.h for s in sources), max(s.plan.w for s in sources),
                                      max(s.stream.size for s in sources), subseq_bits, 0))


def launch(ctx, records: list, info_addr: int, subseq_bits: int = SUBSEQ_BITS, coef_addr: Optional[int] = None, ws=None) -> None:
    """ir_jpeg_decode of the given ir_jpeg_file records on the current stream; info_addr: device uint32 [n]. The scratch is the context's
    workspace unless ws (a device uint8 tensor) is given."""
    from . import _lib as L
    arr = (L.JpegFile * len(records))(*records)
    if ws is None:
        need = int(ctx.lib.ir_workspace_bytes(None, L.STAGE_JPEG_DECODE, len(records), max(r.h for r in records), max(r.w for r in records),
                                              max(r.stream_bytes for r in records), subseq_bits, 0))
        ws = ctx.workspace(need)
    ctx.check(ctx.lib.ir_jpeg_decode(ctx.h, ctx.stream(), arr, len(records), subseq_bits, C.c_void_p(info_addr),
                                     C.c_void_p(coef_addr) if coef_addr else None, L.ptr(ws), ws.numel()), "ir_jpeg_decode")


def decode(ctx, sources: Sequence[JpegSource], subseq_bits: int = SUBSEQ_BITS, pitches: Optional[Sequence[int]] = None, want_coef: bool = False,
           fill: Optional[int] = None):
    """Decode files on the device, the plain way (tests, tools): -> (images as uint8 device tensors [h][pitch], info as a list, coefficients as
    int16 arrays or None). fill: the byte the image buffers hold before the call."""
    import torch
    at, offs = 0, []
    for s in sources:
        offs.append(at)
        at += (s.blob_bytes + 255) & ~255
    host = torch.zeros(at, dtype=torch.uint8)
    for s, o in zip(sources, offs):
        s.pack(host.numpy(), o)
    dev = host.to(ctx.device)
    pitches = list(pitches) if pitches is not None else [3 * s.plan.w for s in sources]
    outs = [torch.full((s.plan.h, p), fill if fill is not None else 0, dtype=torch.uint8, device=ctx.device) for s, p in zip(sources, pitches)]
    info = torch.full((len(sources),), 0x7fffffff, dtype=torch.int32, device=ctx.device)
    coef = torch.zeros(sum(s.blocks for s in sources) * 64, dtype=torch.int16, device=ctx.device) if want_coef else None
    recs = [s.record(dev.data_ptr() + o, out.data_ptr(), p) for s, o, out, p in zip(sources, offs, outs, pitches)]
    launch(ctx, recs, info.data_ptr(), subseq_bits, coef.data_ptr() if want_coef else None)
    torch.cuda.synchronize(ctx.device)
    coefs = None
    if want_coef:
        c, coefs, k = coef.cpu().numpy().reshape(-1, 64), [], 0
        for s in sources:
            coefs.append(c[k:k + s.blocks])
            k += s.blocks
    return outs, [int(v) for v in info.tolist()], coefs
