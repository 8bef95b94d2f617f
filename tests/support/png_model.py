"""CPU restatement of the device PNG encoder's format (csrc/png_encode.hip) in numpy / plain Python: the specification the kernels are
written against and the size yardstick of tests/test_png_gpu.py. Not a byte-for-byte oracle: any prefix code with the same lengths'
cost is as good, and the device may break Huffman ties differently.

  * every scanline: filter type 4 (Paeth), bpp = 3
  * the filtered bytes are cut into chunks of `rows` whole rows; each chunk is ONE dynamic-Huffman block (BTYPE = 10) of literals and
    the end-of-block symbol: HLIT = 257, HDIST = 1 with the one distance length 0, HCLEN = 19 with the code-length alphabet fixed at
    length 4 for symbols 0..15 and 0 for 16..18 (a complete code: each literal length costs 4 plain bits)
  * code lengths limited to 15 by halving the histogram (floor 1) and rebuilding until the longest code fits; should the code of a
    halved histogram cost more on the real one than the fixed code (8 bits for 0..254, 9 for 255 and end-of-block), that code is used
  * every chunk but the last ends with an empty stored block (000, pad, 00 00 FF FF); the last block has BFINAL = 1
  * 2-byte zlib header in front, Adler-32 of the filtered bytes behind
"""
import zlib

import numpy as np

MAXLEN = 15
HEADER_BITS = 17 + 19 * 3 + 257 * 4 + 4
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def paeth_filter(img: np.ndarray) -> np.ndarray:
    """HWC uint8 RGB -> [H][1 + 3 W] uint8: filter-type byte 4, then the Paeth residuals (PNG specification, section 9.4)."""
    h, w, _ = img.shape
    raw = img.reshape(h, 3 * w).astype(np.int16)
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, 3:] = raw[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((h, 3 * w + 1), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = (raw - pred).astype(np.uint8)
    return out


def huffman_lengths(hist):
    """Huffman code lengths of the symbols with a count (two-queue merge; ties by symbol, a leaf before an internal node of equal weight)."""
    leaves = sorted((f, s) for s, f in enumerate(hist) if f)
    n = len(leaves)
    assert n >= 2
    node_w, parent_leaf, parent_node = [], [0] * n, [0] * (n - 1)
    i = j = 0
    for k in range(n - 1):
        w = 0
        for _ in range(2):
            if i < n and (j >= k or leaves[i][0] <= node_w[j]):
                w += leaves[i][0]
                parent_leaf[i] = k
                i += 1
            else:
                w += node_w[j]
                parent_node[j] = k
                j += 1
        node_w.append(w)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[parent_node[k]] + 1
    lens = [0] * len(hist)
    for r, (_, s) in enumerate(leaves):
        lens[s] = depth[parent_leaf[r]] + 1
    return lens


def limited_lengths(hist):
    work = list(hist)
    while True:
        lens = huffman_lengths(work)
        if max(lens) <= MAXLEN:
            break
        work = [max(1, f >> 1) if f else 0 for f in work]
    fixed = [8] * 255 + [9, 9]
    if sum(f * l for f, l in zip(hist, lens)) > sum(f * l for f, l in zip(hist, fixed)):
        return fixed
    return lens


def canonical_codes(lens):
    """RFC 1951 section 3.2.2, then bit-reversed for deflate's LSB-first packing."""
    count = [0] * (MAXLEN + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (MAXLEN + 2), 0
    for l in range(1, MAXLEN + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if not l:
            out.append(0)
            continue
        out.append(int(format(nxt[l], f"0{l}b")[::-1], 2))
        nxt[l] += 1
    return out


def _pack(values, nbits):
    """LSB-first bit string of (value, width) pairs given as two integer arrays -> (uint8 array of single bits)."""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    start = np.concatenate(([0], np.cumsum(nbits)))
    bits = np.zeros(int(start[-1]), np.uint8)
    for b in range(int(nbits.max()) if len(nbits) else 0):
        m = nbits > b
        bits[start[:-1][m] + b] = (values[m] >> b) & 1
    return bits


def encode_chunk(data: np.ndarray, final: bool):
    """One chunk's bytes: header, literals, end-of-block, and the sync flush unless final. Returns (bytes, code lengths)."""
    hist = np.bincount(data, minlength=257).tolist()
    hist[256] = 1
    lens = limited_lengths(hist)
    codes = canonical_codes(lens)
    hv = [1 if final else 0, 2, 0, 0, 15] + [4 if s < 16 else 0 for s in CL_ORDER]
    hn = [1, 2, 5, 5, 4] + [3] * 19
    nib = [int(format(v, "04b")[::-1], 2) for v in range(16)]   # symbol v of the code-length alphabet has the 4-bit code v, sent MSB first
    hv += [nib[l] for l in lens] + [nib[0]]
    hn += [4] * 258
    lens_a, codes_a = np.array(lens), np.array(codes)
    sym = np.concatenate((data.astype(np.int64), [256]))
    bits = np.concatenate((_pack(hv, hn), _pack(codes_a[sym], lens_a[sym])))
    assert HEADER_BITS == sum(hn)
    if not final:
        bits = np.concatenate((bits, np.zeros(3, np.uint8)))
    body = np.packbits(bits, bitorder="little").tobytes()
    return body + (b"" if final else b"\x00\x00\xff\xff"), lens


def encode(img: np.ndarray, rows: int = 8) -> bytes:
    """HWC uint8 RGB -> the zlib stream of the format above."""
    filt = paeth_filter(np.ascontiguousarray(img))
    h = filt.shape[0]
    parts = [b"\x78\x01"]
    for r0 in range(0, h, rows):
        parts.append(encode_chunk(filt[r0:r0 + rows].reshape(-1), r0 + rows >= h)[0])
    parts.append(zlib.adler32(filt.tobytes()).to_bytes(4, "big"))
    return b"".join(parts)


def bound(h: int, w: int, rows: int = 8) -> int:
    """ir_png_bound's derivation: 9 bits per filtered byte, per chunk the header, the end-of-block symbol, the stored block and roundings."""
    chunks = (h + rows - 1) // rows
    return 2 + (9 * h * (3 * w + 1) + 7) // 8 + chunks * ((HEADER_BITS + 9 + 3 + 7 + 7) // 8 + 4 + 1) + 4


# ---- the seeded inputs of the size test (the issue's synthetic A and B: a random low-resolution field, bicubic up, grain of sigma 1)
def synthetic(seed: int, field: int, up: int, sigma: float = 1.0) -> np.ndarray:
    from PIL import Image
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 256, (field, field, 3), dtype=np.uint8)
    big = np.asarray(Image.fromarray(low).resize((field * up, field * up), Image.BICUBIC), np.float32)
    return np.clip(np.rint(big + rng.normal(0.0, sigma, big.shape)), 0, 255).astype(np.uint8)


def synthetic_a() -> np.ndarray:
    return synthetic(11, 32, 32)


def synthetic_b() -> np.ndarray:
    return synthetic(12, 128, 8)
