"""The definition of ir_png_decode (csrc/png_decode.hip) in numpy and plain Python: a PNG file to the pixels Pillow gives,
np.array(Image.open(f).convert("RGB")), byte for byte, and its inflated bytes as zlib.decompress gives them (tests/test_png_decode_cpu.py). The
chunk walk is the product's own (instarevive_amd/png_decode.py: PngSource.open); this file is the decoder behind it, phase by phase in the
kernels' order, and returns every table the kernels leave in their workspace so that the device can be compared against them.

    python tools/png_decode_model.py in.png [out.png] [--compare] [--span_bits 65536]

  find     every bit offset p in 16 .. bits - 17 is tested as the start of a dynamic-Huffman block: BTYPE (bits p + 1, p + 2) = 2, HLIT <= 29,
           HDIST <= 29, the HCLEN + 4 code-length-code lengths a complete code (Kraft sum exactly 1) - the cheap part - then the full header:
           the HLIT + 257 + HDIST + 1 code lengths parse without overrun (a repeat in front of any length, or past the end, is an overrun),
           symbol 256 has a code, and the literal and the distance code are complete by zlib's rule (inftrees.c: never over-subscribed;
           incomplete only as one single code of length 1 or, the distance code, as no code at all). BFINAL may be either.
  spans    cand[k] = the first candidate in bits [k span_bits, (k + 1) span_bits), or 0xffffffff.
  size     entry 0 starts at bit 16, entry k + 1 at cand[k]. A decoder walks blocks of any type from there and counts output bytes. It stops at
           the first block end e with cand[e // span_bits] == e (next = that entry), at the end of a BFINAL block (next = none), or at an error:
           1 block type 3 or a bad dynamic header, 2 a code that does not exist (also literal / length symbols 286, 287 and distance symbols
           30, 31), 3 a read past the stream's bits, 5 LEN != ~NLEN, 6 more output than the image has. Bits behind the stream read as zero.
  chain    from entry 0 along `next`: each entry gets its output offset; an entry's error is the file's; the total must be h (1 + w bpp) (6).
  write    the chain's entries are decoded again: literal[i] and src[i] = i for a literal or stored byte, src[i] = i - distance for a copied
           byte; a distance that reaches before the output's start is error 4.
  resolve  src = src[src] until nothing changes (at most ceil(log2(bytes)) rounds), then byte[i] = literal[src[i]].
  adler    Adler-32 of the bytes against the trailer (7).
  unfilter per row its filter type (above 4: error 8), None / Sub / Up / Average / Paeth on bytes at distance bpp, arithmetic mod 256. The
           kernel runs the rows skewed across lanes; the bytes do not depend on the schedule, so the model goes row by row.
  rgb      grey replicated, alpha dropped.
A file's error is the first one in this order of phases; later phases do not run, and the pixels of such a file are unspecified.
"""
import argparse
import struct
import sys
import zlib
from pathlib import Path

import numpy as np

ROOT = str(Path(__file__).resolve().parent.parent)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from instarevive_amd.png_decode import BPP, NONE, SIGNATURE, SPAN_BITS, PngSource   # noqa: E402

E_HEADER, E_CODE, E_PAST, E_DIST, E_STORED, E_SIZE, E_ADLER, E_FILTER = range(1, 9)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
LUT_BITS = 10


class Bits:
    """The stream as the kernels read it: peek(pos) is 32 bits from bit pos on, LSB first, zero behind the stream."""

    def __init__(self, stream: np.ndarray):
        self.stream = np.ascontiguousarray(stream, dtype=np.uint8)
        self.nbits = 8 * self.stream.size
        padded = np.concatenate([self.stream, np.zeros(24, dtype=np.uint8)]).astype(np.uint64)
        win = np.zeros(self.stream.size + 16, dtype=np.uint64)
        for k in range(8):
            win |= padded[k:k + win.size] << np.uint64(8 * k)
        self.win = win.tolist()

    def peek(self, pos: int) -> int:
        return (self.win[pos >> 3] >> (pos & 7)) & 0xffffffff


def _rev(code: int, n: int) -> int:
    return int(format(code, f"0{n}b")[::-1], 2)


def parse_dynamic(b: Bits, pos: int):
    """The header of a dynamic block behind its three type bits -> (error, pos, lengths, nlen, ndist)."""
    v = b.peek(pos)
    nlen, ndist, ncl = (v & 31) + 257, ((v >> 5) & 31) + 1, ((v >> 10) & 15) + 4
    pos += 14
    if nlen > 286 or ndist > 30:
        return E_HEADER, pos, None, nlen, ndist
    cl, kraft = [0] * 19, 0
    for i in range(ncl):
        cl[CL_ORDER[i]] = b.peek(pos) & 7
        pos += 3
        if cl[CL_ORDER[i]]:
            kraft += 128 >> cl[CL_ORDER[i]]
    if pos > b.nbits:
        return E_PAST, pos, None, nlen, ndist
    if kraft != 128:
        return E_HEADER, pos, None, nlen, ndist
    lut, code = [0] * 128, 0
    for n in range(1, 8):
        for s in range(19):
            if cl[s] == n:
                for k in range(_rev(code, n), 128, 1 << n):
                    lut[k] = s | (n << 5)
                code += 1
        code <<= 1
    total, lens, prev = nlen + ndist, [], 0
    while len(lens) < total:
        v = b.peek(pos)
        e = lut[v & 127]
        s, n = e & 31, e >> 5
        pos += n
        val, rep = s, 1
        if s == 16:
            if not lens:
                return E_HEADER, pos, None, nlen, ndist
            val, rep = prev, 3 + ((v >> n) & 3)
            pos += 2
        elif s == 17:
            val, rep = 0, 3 + ((v >> n) & 7)
            pos += 3
        elif s == 18:
            val, rep = 0, 11 + ((v >> n) & 127)
            pos += 7
        if pos > b.nbits:
            return E_PAST, pos, None, nlen, ndist
        if len(lens) + rep > total:
            return E_HEADER, pos, None, nlen, ndist
        lens += [val] * rep
        prev = val
    lit, dist = lens[:nlen], lens[nlen:]
    kl, kd = sum(32768 >> x for x in lit if x), sum(32768 >> x for x in dist if x)
    if not lit[256] or kl > 32768 or (kl < 32768 and max(lit) != 1) or kd > 32768 or (kd < 32768 and max(dist) > 1):
        return E_HEADER, pos, None, nlen, ndist
    return 0, pos, lens, nlen, ndist


def build(lens):
    """Code lengths -> (the 10-bit table of symbol | length << 9, codes per length, symbols in canonical order)."""
    cnt = [0] * 16
    for x in lens:
        cnt[x] += 1
    cnt[0] = 0
    sym = [s for n in range(1, 16) for s, x in enumerate(lens) if x == n]
    lut, code, at = [0] * (1 << LUT_BITS), 0, 0
    for n in range(1, LUT_BITS + 1):
        for j in range(cnt[n]):
            r = _rev(code + j, n)
            if r < 1 << LUT_BITS:
                for k in range(r, 1 << LUT_BITS, 1 << n):
                    lut[k] = sym[at + j] | (n << 9)
        at, code = at + cnt[n], (code + cnt[n]) << 1
    return lut, cnt, sym


def decode_symbol(v: int, table):
    """-> (length in bits, symbol); length 0: no such code."""
    lut, cnt, sym = table
    e = lut[v & ((1 << LUT_BITS) - 1)]
    if e >> 9:
        return e >> 9, e & 511
    code = first = at = 0
    for n in range(1, 16):
        code |= (v >> (n - 1)) & 1
        if code - cnt[n] < first:
            return n, sym[at + code - first]
        at, first, code = at + cnt[n], (first + cnt[n]) << 1, code << 1
    return 0, 0


_FIXED = None


def walk(b: Bits, pos: int, cand, span_bits: int, n_out: int, out: int = 0, lim=None, lit=None, src=None, blocks=None):
    """Blocks from bit pos on -> (error, end bit, output position, next entry). With lit / src (the writing decode) the output starts at `out`
    and nothing is written at or behind `lim`; every index is asserted in range. blocks: a list that receives (start bit, type) per block."""
    global _FIXED
    write = lit is not None
    cap = lim if write else n_out
    while True:
        if pos + 3 > b.nbits:
            return E_PAST, pos, out, NONE
        start, v = pos, b.peek(pos)
        final, kind = v & 1, (v >> 1) & 3
        pos += 3
        if kind == 3:
            return E_HEADER, pos, out, NONE
        if blocks is not None:
            blocks.append((start, kind))
        if kind == 0:
            pos = (pos + 7) & ~7
            v = b.peek(pos)
            pos += 32
            if pos > b.nbits:
                return E_PAST, pos, out, NONE
            n = v & 0xffff
            if (n ^ 0xffff) != v >> 16:
                return E_STORED, pos, out, NONE
            if n > (b.nbits - pos) // 8:
                return E_PAST, pos, out, NONE
            if n > cap - out:
                return E_SIZE, pos, out, NONE
            if write:
                assert 0 <= out and out + n <= len(lit) and (pos >> 3) + n <= b.stream.size
                lit[out:out + n] = b.stream[pos >> 3:(pos >> 3) + n]
                src[out:out + n] = np.arange(out, out + n, dtype=np.uint32)
            out, pos = out + n, pos + 8 * n
        else:
            if kind == 1:
                if _FIXED is None:
                    _FIXED = (build(FIXED_LENS), build([5] * 30))
                tl, td = _FIXED
            else:
                err, pos, lens, nlen, _ = parse_dynamic(b, pos)
                if err:
                    return err, pos, out, NONE
                tl, td = build(lens[:nlen]), build(lens[nlen:])
            while True:
                v = b.peek(pos)
                n, s = decode_symbol(v, tl)
                if not n:
                    return E_CODE, pos, out, NONE
                pos += n
                if pos > b.nbits:
                    return E_PAST, pos, out, NONE
                if s < 256:
                    if out >= cap:
                        return E_SIZE, pos, out, NONE
                    if write:
                        assert 0 <= out < len(lit)
                        lit[out], src[out] = s, out
                    out += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    return E_CODE, pos, out, NONE
                length = LEN_BASE[s - 257] + ((v >> n) & ((1 << LEN_EXTRA[s - 257]) - 1))
                pos += LEN_EXTRA[s - 257]
                v = b.peek(pos)
                n, s = decode_symbol(v, td)
                if not n or s > 29:
                    return E_CODE, pos, out, NONE
                dist = DIST_BASE[s] + ((v >> n) & ((1 << DIST_EXTRA[s]) - 1))
                pos += n + DIST_EXTRA[s]
                if pos > b.nbits:
                    return E_PAST, pos, out, NONE
                if length > cap - out:
                    return E_SIZE, pos, out, NONE
                if write:
                    assert 0 <= out and out + length <= len(src)
                    idx = np.arange(out, out + length, dtype=np.int64)
                    if dist > out:
                        src[out:out + length], lit[out:out + length] = idx, 0
                        return E_DIST, pos, out, NONE
                    assert (idx - dist >= 0).all()
                    src[out:out + length] = idx - dist
                out += length
        if final:
            return 0, pos, out, NONE
        sp = pos // span_bits
        if sp < len(cand) and cand[sp] == pos:
            return 0, pos, out, sp + 1


def candidates(b: Bits) -> np.ndarray:
    """Every bit offset that passes the finder's test, ascending."""
    nbits = b.nbits
    bits = np.concatenate([np.unpackbits(b.stream, bitorder="little"), np.zeros(128, dtype=np.uint8)]).astype(np.int32)

    def field(off, n):   # the n-bit number at p + off, for every p
        return sum(bits[off + k:off + k + nbits] << k for k in range(n))

    p = np.arange(nbits)
    ncl = field(13, 4) + 4
    ok = (p >= 16) & (p + 17 <= nbits) & (field(1, 2) == 2) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    kraft = np.zeros(nbits, dtype=np.int32)
    for i in range(19):
        n = field(17 + 3 * i, 3)
        kraft += np.where((i < ncl) & (n > 0), 128 >> n, 0)
    ok &= (kraft == 128) & (p + 17 + 3 * ncl <= nbits)
    return np.array([q for q in np.flatnonzero(ok).tolist() if parse_dynamic(b, q + 3)[0] == 0], dtype=np.int64)


def unfilter(raw: np.ndarray, h: int, w: int, bpp: int):
    """The inflated bytes -> (error, the unfiltered bytes [h][w bpp], the rows' filter types)."""
    rb = w * bpp
    rows = raw.reshape(h, rb + 1)
    types = rows[:, 0].copy()
    if (types > 4).any():
        return E_FILTER, None, types
    out, prev = np.zeros((h, rb), dtype=np.uint8), np.zeros(rb, dtype=np.uint8)
    for y in range(h):
        x, t = rows[y, 1:], int(types[y])
        if t == 0:
            cur = x.copy()
        elif t == 1:
            cur = np.cumsum(x.reshape(w, bpp).astype(np.uint32), axis=0).astype(np.uint8).reshape(rb)
        elif t == 2:
            cur = x + prev
        else:
            xs, ps, c = x.tolist(), prev.tolist(), [0] * rb
            for i in range(rb):
                a = c[i - bpp] if i >= bpp else 0
                if t == 3:
                    c[i] = (xs[i] + ((a + ps[i]) >> 1)) & 255
                else:
                    up, ul = ps[i], ps[i - bpp] if i >= bpp else 0
                    pa, pb, pc = abs(up - ul), abs(a - ul), abs(a + up - 2 * ul)
                    c[i] = (xs[i] + (a if pa <= pb and pa <= pc else up if pb <= pc else ul)) & 255
            cur = np.array(c, dtype=np.uint8)
        out[y] = prev = cur
    return 0, out, types


def to_rgb(px: np.ndarray, h: int, w: int, bpp: int) -> np.ndarray:
    px = px.reshape(h, w, bpp)
    return np.ascontiguousarray(np.repeat(px[:, :, :1], 3, axis=2) if bpp < 3 else px[:, :, :3])


def decode(source: PngSource, span_bits: int = SPAN_BITS) -> dict:
    """Every phase, in the kernel's order. Keys: valid (all candidates), cand, end / next / length / status (per entry; 0xffffffff for an entry
    without a candidate), chain, offset, total, error, blocks (start bit, type) along the chain, lit, src0 (as written), src (resolved), rounds
    (squaring rounds that changed something), bytes, adler, types (the rows' filter types), pixels (uint8 [h][w][3], or None with an error)."""
    b = Bits(source.stream)
    n_out, spans = source.inflated, -(-b.nbits // span_bits)
    valid = candidates(b)
    cand = np.full(spans, NONE, dtype=np.uint32)
    for q in valid[::-1].tolist():
        cand[q // span_bits] = q
    entries = spans + 1
    end, nxt, status = (np.full(entries, NONE, dtype=np.uint32) for _ in range(3))
    length = np.zeros(entries, dtype=np.uint32)
    for e in range(entries):
        start = 16 if e == 0 else int(cand[e - 1])
        if start != NONE:
            status[e], end[e], length[e], nxt[e] = walk(b, start, cand, span_bits, n_out)
    r = dict(valid=valid, cand=cand, end=end, next=nxt, length=length, status=status, pixels=None, blocks=[], rounds=0, types=None)
    chain, offset, e, off, err = [], np.zeros(entries, dtype=np.uint32), 0, 0, 0
    for _ in range(entries):
        if status[e]:
            err = E_HEADER if status[e] == NONE else int(status[e])
            break
        chain.append(e)
        offset[e] = off
        if length[e] > n_out - off:
            err = E_SIZE
            break
        off += int(length[e])
        if nxt[e] == NONE:
            break
        assert e < nxt[e] < entries
        e = int(nxt[e])
    if not err and off != n_out:
        err = E_SIZE
    r.update(chain=np.array(chain, dtype=np.uint32), offset=offset, total=off, error=err)
    if err:
        return r
    lit, src = np.zeros(n_out, dtype=np.uint8), np.full(n_out, NONE, dtype=np.uint32)
    for e in chain:
        start = 16 if e == 0 else int(cand[e - 1])
        st, at, out, to = walk(b, start, cand, span_bits, n_out, int(offset[e]), int(offset[e] + length[e]), lit, src, r["blocks"])
        if st:
            r["error"] = st
            return r
        assert (at, out - int(offset[e]), to) == (int(end[e]), int(length[e]), int(nxt[e]))
    assert (src <= np.arange(n_out)).all()
    r.update(lit=lit, src0=src.copy())
    src = src.astype(np.int64)
    while True:
        again = src[src]
        if np.array_equal(again, src):
            break
        src, r["rounds"] = again, r["rounds"] + 1
    assert r["rounds"] <= max(1, (n_out - 1).bit_length())
    r.update(src=src.astype(np.uint32), bytes=lit[src])
    r["adler"] = zlib.adler32(r["bytes"].tobytes())
    if r["adler"] != source.adler:
        r["error"] = E_ADLER
        return r
    err, px, r["types"] = unfilter(r["bytes"], source.h, source.w, source.bpp)
    if err:
        r["error"] = err
        return r
    r["pixels"] = to_rgb(px, source.h, source.w, source.bpp)
    return r


# ---------------------------------------------------------------- a PNG writer for the tests
def filter_rows(px: np.ndarray, types) -> bytes:
    """px uint8 [h][w][bpp], one filter type per row -> the filtered scanlines, each behind its type byte (a type above 4 is written as it is,
    with the row unfiltered)."""
    h, w, bpp = px.shape
    cur = px.reshape(h, w * bpp).astype(np.int32)
    a = np.zeros_like(cur)
    a[:, bpp:] = cur[:, :-bpp]
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    ul = np.zeros_like(cur)
    ul[:, bpp:] = up[:, :-bpp]
    pa, pb, pc = abs(up - ul), abs(a - ul), abs(a + up - 2 * ul)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, ul))
    pred = [np.zeros_like(cur), a, up, (a + up) >> 1, paeth]
    rows = []
    for y, t in enumerate(types):
        rows.append(bytes([t]) + ((cur[y] - pred[t][y] if t <= 4 else cur[y]) & 255).astype(np.uint8).tobytes())
    return b"".join(rows)


def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_of_stream(h: int, w: int, color_type: int, z: bytes, idat: int = 65536, depth: int = 8, interlace: int = 0, extra=()) -> bytes:
    """A PNG file around the zlib stream z, its IDAT chunks of `idat` bytes; extra: chunks (kind, body) between IHDR and the first IDAT."""
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))]
    out += [chunk(k, body) for k, body in extra]
    out += [chunk(b"IDAT", z[i:i + idat]) for i in range(0, len(z), idat)]
    return b"".join(out + [chunk(b"IEND", b"")])


def deflate(raw: bytes, level: int = 6, mem_level: int = 8, strategy: int = zlib.Z_DEFAULT_STRATEGY, flush_every: int = 0) -> bytes:
    """zlib.compressobj over raw; flush_every: a Z_FULL_FLUSH after every so many bytes."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    if not flush_every:
        return c.compress(raw) + c.flush()
    parts = []
    for i in range(0, len(raw), flush_every):
        parts += [c.compress(raw[i:i + flush_every]), c.flush(zlib.Z_FULL_FLUSH)]
    return b"".join(parts) + c.flush()


def write_png(px: np.ndarray, types, idat: int = 65536, **zargs) -> bytes:
    """px uint8 [h][w][1 | 2 | 3 | 4] (grey, grey + alpha, RGB, RGBA), a filter type per row, deflate()'s arguments."""
    h, w, bpp = px.shape
    color_type = {v: k for k, v in BPP.items()}[bpp]
    return png_of_stream(h, w, color_type, deflate(filter_rows(px, types), **zargs), idat)


class BitWriter:
    """Deflate's bit order: fields LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int) -> None:
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc, self.n = self.acc >> 8, self.n - 8

    def code(self, code: int, bits: int) -> None:
        self.put(_rev(code, bits), bits)

    def align(self) -> None:
        if self.n:
            self.put(0, 8 - self.n)

    def stored(self, data: bytes, final: bool = False) -> None:
        self.put(int(final), 1)
        self.put(0, 2)
        self.align()
        self.put(len(data), 16)
        self.put(len(data) ^ 0xffff, 16)
        self.out += data

    def fixed_symbol(self, s: int) -> None:   # a literal / length symbol of the fixed code (RFC 1951, 3.2.6)
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xc0 + s - 280, 8)

    def fixed_match(self, length: int, dist: int) -> None:
        s = max(i for i in range(29) if LEN_BASE[i] <= length)
        self.fixed_symbol(257 + s)
        self.put(length - LEN_BASE[s], LEN_EXTRA[s])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(d, 5)
        self.put(dist - DIST_BASE[d], DIST_EXTRA[d])

    def zlib_stream(self, raw: bytes) -> bytes:
        """The bits so far as a zlib stream whose trailer is the Adler-32 of raw."""
        self.align()
        return b"\x78\x01" + bytes(self.out) + struct.pack(">I", zlib.adler32(raw))


def main():
    ap = argparse.ArgumentParser(description="decode a PNG through the definition of ir_png_decode")
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?", help="where to save the pixels (PNG)")
    ap.add_argument("--compare", action="store_true", help="compare with Pillow's decode and zlib's inflate")
    ap.add_argument("--span_bits", type=int, default=SPAN_BITS)
    args = ap.parse_args()
    data = Path(args.src).read_bytes()
    source, why = PngSource.open(data)
    if source is None:
        print(f"{args.src}: not taken ({why})")
        return 2
    r = decode(source, args.span_bits)
    kinds = [k for _, k in r["blocks"]]
    print(f"{args.src}: {source.w} x {source.h}, colour type {source.color_type}, {source.stream.size} stream bytes, {len(r['valid'])} candidates, "
          f"{len(r['chain'])} chain entries, blocks stored / fixed / dynamic {kinds.count(0)} / {kinds.count(1)} / {kinds.count(2)}, "
          f"{r['rounds']} squaring rounds, error {r['error']}")
    if r["error"]:
        return 1
    from PIL import Image
    if args.compare:
        ref = np.array(Image.open(args.src).convert("RGB"))
        same = np.array_equal(ref, r["pixels"]) and r["bytes"].tobytes() == zlib.decompressobj().decompress(source.stream.tobytes())
        print("equal to Pillow and zlib" if same else "DIFFERS from Pillow or zlib")
        if not same:
            return 1
    if args.dst:
        Image.fromarray(r["pixels"]).save(args.dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
