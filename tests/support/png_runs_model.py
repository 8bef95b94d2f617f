"""CPU restatement of the run mode of the device PNG encoder (ir_png_encode_runs, csrc/png_encode.hip) in numpy / plain Python, next to
png_model.py, which states the literal-only mode and is imported for everything the two share. The stream's LENGTH is what the device has to
reproduce: every prefix code with the same lengths costs the same, and the lengths come from one deterministic construction.

  * the filtered stream, the chunks of `rows` whole rows, the zlib header, the Adler-32 and the empty stored block behind every chunk but the
    last are png_model's
  * inside a chunk the flattened bytes (filter-type bytes included) are cut into their maximal runs of equal bytes; a run may cross rows, never
    the chunk's boundary. A run of R bytes is coded as one literal, then (R - 1) // 258 matches of length 258 at distance 1, then the remainder
    r = (R - 1) % 258 as one match of length r if r >= MIN, as r literals otherwise (a match longer than its distance is plain deflate, RFC
    1951 section 3.2.3). So a byte decides alone what it emits from where its run starts and ends: a literal, a match, or nothing
  * a run-coded chunk is ONE dynamic-Huffman block: HLIT = 286 literal / length codes with RFC 1951's length extra bits, HDIST = 1: distance
    code 0 with length 1, so every match pays one distance bit (one used distance code is sent with one bit, section 3.2.7)
  * the literal / length code: Huffman lengths of the chunk's histogram (end-of-block counted once), limited to 15 by png_model's halving
  * the code-length section: HCLEN = 19 with a FIXED complete code for the code-length alphabet - 3 bits for symbol 18, 4 bits for 0, 3 .. 11
    and 17, 5 bits for 1, 2, 12 .. 15, none for 16 - and the 287 lengths (286 + the distance's) sent greedily: a stretch of n zeros as
    symbol 18 (11 .. 138 zeros, 7 extra bits) while n >= 11, then symbol 17 (3 .. 10 zeros, 3 extra bits) if n >= 3, else n plain zeros;
    every other length as its own symbol. A flat chunk's header takes about 25 bytes where the literal-only mode's takes 139
  * per chunk the bit cost of this block and of png_model's literal-only block (header, symbols, end-of-block) are compared and the cheaper
    one is emitted, the literal-only block on a tie: the stream is never longer than png_model.encode's, and png_model.bound holds

MIN = 6, chosen on the 512 x 512 size cases of tests/support/png_runs_cases.py (bytes of the stream; a short match pays a length code and
the distance bit where the literals it replaces, mostly zeros, cost 1 - 2 bits each):
                     literal-only     MIN 3     MIN 4     MIN 5     MIN 6     MIN 8    MIN 12
    constant              107 587     3 014     3 014     3 014     3 014     3 014     3 014
    sky                   109 748    18 193    18 193    17 402    17 402    17 808    17 758
    flat_regions          110 075     9 816     9 816     9 816     9 785     9 785     9 812
    photo                 332 194   325 733   325 164   325 014   324 948   324 921   324 919
    sky_over_photo        221 930   172 905   172 637   172 177   172 141   172 330   172 304
6 is the smallest on the three cases that depend on it at all and within 30 bytes of the best on photo.
"""
import zlib

import numpy as np

from tests.support import png_model as M

MIN = 6
MAX_MATCH = 258
NSYM = 286
EOB = 256
# the code-length alphabet's fixed code: Kraft sum 1/8 + 11/16 + 6/32 = 1
CL_LENS = [4, 5, 5] + [4] * 9 + [5] * 4 + [0, 4, 3]


def length_symbol(length):
    """Match length 3 .. 258 -> (symbol 257 .. 285, extra bit count, extra value), RFC 1951 section 3.2.5. Works on arrays."""
    l = np.asarray(length, np.int64) - 3
    eb = np.where(l < 8, 0, np.floor(np.log2(np.maximum(l, 1))).astype(np.int64) - 2)
    sym = np.where(l < 8, 257 + l, 261 + 4 * eb + ((l >> eb) & 3))
    extra = l & ((1 << eb) - 1)
    full = l == MAX_MATCH - 3
    return np.where(full, 285, sym), np.where(full, 0, eb), np.where(full, 0, extra)


def tokens(data: np.ndarray, minimum: int = MIN):
    """The chunk's parse: (positions of the literals, positions of the match heads, their lengths)."""
    n = len(data)
    flag = np.ones(n, bool)
    flag[1:] = data[1:] != data[:-1]
    starts = np.flatnonzero(flag)
    ends = np.append(starts[1:], n)
    lit, head, length = [starts], [], []
    rest = ends - starts - 1
    full = rest // MAX_MATCH
    for s, f, r in zip(starts[rest > 0].tolist(), full[rest > 0].tolist(), (rest % MAX_MATCH)[rest > 0].tolist()):
        head.append(s + 1 + MAX_MATCH * np.arange(f))
        length.append(np.full(f, MAX_MATCH))
        at = s + 1 + MAX_MATCH * f
        if r >= minimum:
            head.append([at])
            length.append([r])
        else:
            lit.append(at + np.arange(r))
    cat = lambda parts: np.concatenate([np.asarray(p, np.int64) for p in parts]) if parts else np.zeros(0, np.int64)
    return np.sort(cat(lit)), cat(head), cat(length)


def limited_lengths(hist):
    """png_model.limited_lengths without the fixed code: a code that costs too much loses the chunk to the literal-only block anyway."""
    work = list(hist)
    while True:
        lens = M.huffman_lengths(work)
        if max(lens) <= M.MAXLEN:
            return lens
        work = [max(1, f >> 1) if f else 0 for f in work]


def header_fields(lens, final: bool):
    """(values, widths) of the block header of the 286 literal / length code lengths `lens`."""
    cl_codes = M.canonical_codes(CL_LENS)
    hv = [1 if final else 0, 2, NSYM - 257, 0, 15] + [CL_LENS[s] for s in M.CL_ORDER]
    hn = [1, 2, 5, 5, 4] + [3] * 19
    seq = list(lens) + [1]
    i = 0
    while i < len(seq):
        v, k = seq[i], i
        while k < len(seq) and seq[k] == v:
            k += 1
        n = k - i if v == 0 else 1
        i += n
        if v:
            hv.append(cl_codes[v]); hn.append(CL_LENS[v])
            continue
        while n >= 11:
            t = min(n, 138)
            hv += [cl_codes[18], t - 11]; hn += [CL_LENS[18], 7]
            n -= t
        if n >= 3:
            hv += [cl_codes[17], n - 3]; hn += [CL_LENS[17], 3]
            n = 0
        hv += [cl_codes[0]] * n; hn += [CL_LENS[0]] * n
    return hv, hn


def encode_chunk(data: np.ndarray, final: bool, minimum: int = MIN):
    """One chunk as a run-coded block: (bytes with the sync flush unless final, the block's bits up to and including end-of-block)."""
    lit, head, length = tokens(data, minimum)
    lsym, leb, lextra = length_symbol(length)
    hist = (np.bincount(data[lit], minlength=NSYM) + np.bincount(lsym, minlength=NSYM)).tolist()
    hist[EOB] = 1
    lens = limited_lengths(hist)
    codes = M.canonical_codes(lens)
    lens_a, codes_a = np.array(lens, np.int64), np.array(codes, np.int64)
    # one (value, width) per token in stream order; a match is its length code, the extra bits, and the distance code's single 0 bit
    pos = np.concatenate((lit, head))
    val = np.concatenate((codes_a[data[lit]], codes_a[lsym] | (lextra << lens_a[lsym])))
    wid = np.concatenate((lens_a[data[lit]], lens_a[lsym] + leb + 1))
    order = np.argsort(pos, kind="stable")
    hv, hn = header_fields(lens, final)
    bits = np.concatenate((M._pack(hv, hn), M._pack(np.append(val[order], codes[EOB]), np.append(wid[order], lens[EOB]))))
    nbits = len(bits)
    if not final:
        bits = np.concatenate((bits, np.zeros(3, np.uint8)))
    return np.packbits(bits, bitorder="little").tobytes() + (b"" if final else b"\x00\x00\xff\xff"), nbits


def literal_bits(data: np.ndarray) -> int:
    """The bits of png_model's literal-only block of the chunk: header, literals, end-of-block."""
    hist = np.bincount(data, minlength=257).tolist()
    hist[256] = 1
    return M.HEADER_BITS + sum(f * l for f, l in zip(hist, M.limited_lengths(hist)))


def encode(img: np.ndarray, rows: int = 8, minimum: int = MIN, choices=None) -> bytes:
    """HWC uint8 RGB -> the zlib stream of the format above. choices: a list that receives True per run-coded chunk."""
    filt = M.paeth_filter(np.ascontiguousarray(img))
    h = filt.shape[0]
    parts = [b"\x78\x01"]
    for r0 in range(0, h, rows):
        data, final = filt[r0:r0 + rows].reshape(-1), r0 + rows >= h
        body, nbits = encode_chunk(data, final, minimum)
        runs = nbits < literal_bits(data)
        parts.append(body if runs else M.encode_chunk(data, final)[0])
        if choices is not None:
            choices.append(runs)
    parts.append(zlib.adler32(filt.tobytes()).to_bytes(4, "big"))
    return b"".join(parts)
