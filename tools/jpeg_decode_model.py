"""The definition of ir_jpeg_decode (csrc/jpeg_decode.hip) in numpy and plain Python: a baseline JPEG file to the pixels Pillow gives,
np.array(Image.open(f).convert("RGB")), byte for byte (tests/test_jpeg_decode_cpu.py). The marker parser and the vectorised byte pass are the
product's own (instarevive_amd/jpeg_decode.py: parse, entropy_segments); this file restates the byte pass as a loop, and is the decoder behind it.
The pixel arithmetic - libjpeg's ISLOW inverse DCT, the colour constants - is tools/degrade_folder.py's.

    python tools/jpeg_decode_model.py in.jpg [out.png] [--compare] [--parallel 1024]

The rules, each libjpeg's:
  scan     one interleaved scan; an MCU is hs x vs luma blocks (rows first) then Cb then Cr, or one block for a grey file (a single-component scan
           has 8 x 8 MCUs whatever its sampling factors say). Restart intervals of `restart` MCUs in raster order, each a bit stream of its own:
           the predictors reset, the last byte is padded with 1-bits.
  coding   a DC symbol is the size n (<= 11) of the difference, then n value bits (a first bit of 0: the value minus 2^n - 1); an AC symbol is
           run << 4 | size: run zeros, then a value of `size` bits; 0xF0 is sixteen zeros, any other symbol of size 0 ends the block.
  state    (bit position, block of the MCU, coefficient index 0 .. 63; 0: a DC symbol comes next). At an MCU boundary with fewer than 8 bits
           left, all of them 1, the interval is over. Decoding goes on until the interval's bits are used up - how many blocks it should hold
           is checked afterwards, so that a subsequence, which cannot know, decodes like the sequential walk.
  errors   1 invalid code (also a DC size above 11), 2 coefficient index past 63, 3 a symbol that reads past the interval's bit count, 4 wrong
           block count for the interval (or an end inside an MCU). A file's error is that of its first interval that has one.
  pixels   dequantise, jidctint.c down the columns and along the rows, + 128, clamp to 0 .. 255 (libjpeg's wrap-around for absurd coefficients
           is not reproduced: no encoder's output reaches it); h2v2 fancy upsampling ((3 near + far) both ways, + 8 / + 7, >> 4) and h2v1 fancy
           upsampling ((3 c + left + 1) >> 2 for even, (3 c + right + 2) >> 2 for odd output columns; the first and the last column copy the
           sample) on the TRUE chroma size ceil(w / 2) [x ceil(h / 2)]; jdcolor.c's YCbCr -> RGB; the crop to h x w.
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = str(Path(__file__).resolve().parent.parent)
sys.path.insert(0, str(Path(__file__).resolve().parent))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from degrade_folder import _fix, _idct_pass   # noqa: E402
from instarevive_amd.jpeg_decode import ZIGZAG, Plan, entropy_segments, parse   # noqa: E402,F401

E_CODE, E_INDEX, E_PAST, E_COUNT = 1, 2, 3, 4
COUNTS = ("zrl", "last_coef", "stuffed", "restart_markers", "negative_dc", "long_codes")


class DecodeError(ValueError):
    def __init__(self, cls, interval):
        super().__init__(f"error class {cls} in restart interval {interval}")
        self.cls, self.interval = cls, interval


def entropy_segments_loop(plan: Plan):
    """entropy_segments byte by byte."""
    out, table, cur, k, scan, i = bytearray(), [], bytearray(), 0, plan.scan, 0

    def close():
        table.append((len(out), 8 * len(cur)))
        out.extend(cur + bytes(-len(cur) % 4))

    while i < len(scan):
        b = scan[i]
        nxt = scan[i + 1] if i + 1 < len(scan) else 0xFF   # the scan ends in front of a marker
        if b != 0xFF:
            cur.append(b)
        elif nxt == 0:
            cur.append(0xFF)
            i += 1
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != k % 8:
                return None
            close()
            cur, k, i = bytearray(), k + 1, i + 1
        elif nxt != 0xFF:
            raise AssertionError("a marker inside the scan")
        i += 1
    close()
    if len(table) != plan.n_intervals:
        return None
    return np.frombuffer(bytes(out) or bytes(4), dtype=np.uint8), np.array(table, dtype=np.uint32)


def _code_lists(plan: Plan):
    """Per Huffman table (DC 0, DC 1, AC 0, AC 1) a dict {(length, code): symbol}."""
    tabs = [None] * 4
    for (cls, tid), (counts, vals) in plan.huff.items():
        d, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(counts[l - 1]):
                d[(l, code)] = vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        tabs[2 * cls + tid] = d
    return tabs


class _Interval:
    """One restart interval as a string of '0' / '1' and the symbol decoder on it, memoised per (bit position, table)."""

    def __init__(self, plan, tabs, data: np.ndarray, bits: int):
        self.bits = bits
        self.s = "".join(format(b, "08b") for b in data.tobytes())[:bits]
        self.tabs, self.memo = tabs, {}
        self.bpm = plan.blocks_per_mcu
        ny = plan.hs * plan.vs
        self.comp = [0 if plan.comps == 1 or b < ny else b - ny + 1 for b in range(self.bpm)]
        self.td, self.ta = plan.td, plan.ta

    def symbol(self, p: int, t: int):
        """(bits used, symbol, value) of the symbol of table t at bit p, or the error class."""
        key = (p, t)
        r = self.memo.get(key)
        if r is None:
            r = self.memo[key] = self._symbol(p, t)
        return r

    def _symbol(self, p, t):
        s, tab = self.s, self.tabs[t]
        window = s[p:p + 16].ljust(16, "0")   # bits past the interval read as zero
        for l in range(1, 17):
            sym = tab.get((l, int(window[:l], 2)))
            if sym is not None:
                break
        else:
            return E_CODE
        if t < 2 and sym > 11:
            return E_CODE
        size = sym if t < 2 else sym & 15
        if p + l + size > self.bits:
            return E_PAST
        v = 0
        if size:
            v = int(s[p + l:p + l + size], 2)
            if v < 1 << (size - 1):
                v -= (1 << size) - 1
        return l + size, sym, v, l

    def step(self, p, b, k, sink=None, counts=None):
        """One symbol from state (p, b, k): the next state and whether a block ended, or the error class. sink(k, value) takes a value."""
        t = self.td[self.comp[b]] if k == 0 else 2 + self.ta[self.comp[b]]
        r = self.symbol(p, t)
        if isinstance(r, int):
            return r
        used, sym, v, l = r
        if counts is not None and l > 9:
            counts["long_codes"] += 1
        p += used
        if k == 0:
            if sink:
                sink(0, v)
            if counts is not None and v < 0:
                counts["negative_dc"] += 1
            return p, b, 1, False
        if sym & 15 == 0:
            if sym == 0xF0:
                if counts is not None:
                    counts["zrl"] += 1
                return (p, b, k + 16, False) if k + 16 <= 63 else E_INDEX
            return p, (b + 1) % self.bpm, 0, True
        k += sym >> 4
        if k > 63:
            return E_INDEX
        if sink:
            sink(k, v)
        if k == 63:
            if counts is not None:
                counts["last_coef"] += 1
            return p, (b + 1) % self.bpm, 0, True
        return p, b, k + 1, False

    def padded_end(self, p, b, k):
        """At an MCU boundary with fewer than 8 bits left, all of them 1."""
        return k == 0 and b == 0 and self.bits - p < 8 and "0" not in self.s[p:]

    def run(self, state, end, sink=None, counts=None):
        """Decode from `state` to the first symbol boundary at or behind `end`: (exit state, blocks finished, error class or 0). A symbol that
        cannot be decoded ends the run in the state the right neighbour guesses, (end, 0, 0): a guess that went wrong must not keep the
        subsequences to its right from synchronising. sink(block, k, value) takes the values; block counts from 0 at the block `state` stands in."""
        p, b, k = state
        n = 0
        put = (lambda kk, v: sink(n, kk, v)) if sink else None
        while p < end:
            if self.padded_end(p, b, k):
                p = self.bits
                break
            r = self.step(p, b, k, put, counts)
            if isinstance(r, int):
                return (end, 0, 0), n, r
            p, b, k, done = r
            n += done
        return (p, b, k), n, 0


def _intervals(plan: Plan, segments=None):
    """segments: (stream, interval table) in place of entropy_segments(plan)'s - what a test has damaged."""
    stream, table = segments if segments is not None else entropy_segments(plan)
    tabs = _code_lists(plan)
    return [_Interval(plan, tabs, stream[int(o):int(o) + int(bits) // 8], int(bits)) for o, bits in table]


def _finish(plan: Plan, coef: np.ndarray) -> np.ndarray:
    """DC differences to values: the prefix sum per component inside every restart interval. int16 like the device's array."""
    bpm, ny = plan.blocks_per_mcu, plan.hs * plan.vs
    per = (plan.restart or (len(coef) // bpm)) * bpm
    for j in range(plan.n_intervals):
        blk = coef[j * per:(j + 1) * per].reshape(-1, bpm, 64)
        for first, count in (((0, ny), (ny, 1), (ny + 1, 1)) if plan.comps == 3 else ((0, 1),)):
            dc = blk[:, first:first + count, 0]
            dc[...] = np.cumsum(dc.reshape(-1).astype(np.int64)).astype(np.int16).reshape(dc.shape)
    return coef


def _check_end(plan, j, state, blocks, err=0):
    if err:
        raise DecodeError(err, j)
    p, b, k = state
    if b or k or blocks != plan.interval_mcus(j) * plan.blocks_per_mcu:
        raise DecodeError(E_COUNT, j)


def decode_coefficients(plan: Plan, counts=None, segments=None) -> np.ndarray:
    """The sequential decode: int16 [blocks][64] in natural order, DC summed, blocks in scan order. Raises DecodeError. counts: a dict that
    receives COUNTS."""
    my, mx = plan.mcu_grid
    bpm = plan.blocks_per_mcu
    coef = np.zeros((my * mx * bpm, 64), dtype=np.int16)
    if counts is not None:
        counts.update({k: 0 for k in COUNTS})
        scan = np.frombuffer(plan.scan, dtype=np.uint8)
        counts["stuffed"] = int(np.count_nonzero((scan[:-1] == 0xFF) & (scan[1:] == 0)))
        counts["restart_markers"] = plan.n_intervals - 1
    for j, iv in enumerate(_intervals(plan, segments)):
        base = j * plan.restart * bpm
        limit = base + plan.interval_mcus(j) * bpm

        def sink(n, k, v, base=base, limit=limit):
            if base + n < limit:
                coef[base + n, ZIGZAG[k]] = v
        state, blocks, err = iv.run((0, 0, 0), iv.bits, sink, counts)
        _check_end(plan, j, state, blocks, err)
    return _finish(plan, coef)


def last_mcu_start(plan: Plan, j: int) -> int:
    """The bit at which the last MCU of restart interval j starts (for tests that cut it off)."""
    iv = _intervals(plan)[j]
    state, blocks, want = (0, 0, 0), 0, (plan.interval_mcus(j) - 1) * plan.blocks_per_mcu
    while blocks < want:
        *state, done = iv.step(*state)
        blocks += done
    return state[0]


def parallel_entropy_model(plan: Plan, subseq_bits: int):
    """The device algorithm: subsequences of subseq_bits bits inside each restart interval, the first of an interval in the known state, the others
    guessing (their first bit, block 0, coefficient 0). Round r gives every subsequence its left neighbour's exit state of round r - 1 as its entry
    state and decodes it again where that changed; the rounds end when nothing changes - the entry states are then the sequential walk's. An
    exclusive scan of the blocks finished per subsequence gives each its first block, and a second decode from the synchronised entry states
    writes the coefficients. -> (decode_coefficients' array, the rounds in which something changed - the most over the intervals)."""
    if subseq_bits % 32 or not 128 <= subseq_bits <= 4096:
        raise ValueError("subseq_bits: a multiple of 32 in 128 .. 4096")
    my, mx = plan.mcu_grid
    bpm, S = plan.blocks_per_mcu, subseq_bits
    coef = np.zeros((my * mx * bpm, 64), dtype=np.int16)
    rounds = 0
    for j, iv in enumerate(_intervals(plan)):
        n = max(1, -(-iv.bits // S))
        ends = [min((i + 1) * S, iv.bits) for i in range(n)]
        entry = [(0, 0, 0)] + [(i * S, 0, 0) for i in range(1, n)]
        memo = {}   # (subsequence, entry state) -> its run: guesses that have become one walk are decoded once

        def run(i):
            key = (i, entry[i])
            if key not in memo:
                memo[key] = iv.run(entry[i], ends[i])
            return memo[key]
        out = [run(i) for i in range(n)]
        r = 0
        while True:
            dirty = [i for i in range(1, n) if out[i - 1][0] != entry[i]]
            if not dirty:
                break
            for i in dirty:
                entry[i] = out[i - 1][0]
            for i in dirty:
                out[i] = run(i)
            r += 1
        rounds = max(rounds, r)
        first = np.concatenate([[0], np.cumsum([o[1] for o in out])])
        base = j * plan.restart * bpm
        limit = base + plan.interval_mcus(j) * bpm
        err = 0
        for i in range(n):
            def sink(nb, k, v, b0=base + int(first[i])):
                if b0 + nb < limit:
                    coef[b0 + nb, ZIGZAG[k]] = v
            err = err or iv.run(entry[i], ends[i], sink)[2]
        _check_end(plan, j, out[-1][0], int(first[-1]), err)
    return _finish(plan, coef), rounds


def file_error(plan: Plan, segments=None) -> int:
    """info of ir_jpeg_decode for this file: 0, or the error class of its first interval that has one."""
    try:
        decode_coefficients(plan, segments=segments)
    except DecodeError as e:
        return e.cls
    return 0


def component_planes(plan: Plan, coef: np.ndarray):
    """The sample planes on the MCU grid: [Y] or [Y, Cb, Cr], uint8."""
    my, mx = plan.mcu_grid
    bpm, ny = plan.blocks_per_mcu, plan.hs * plan.vs
    blocks = coef.astype(np.int64).reshape(my, mx, bpm, 8, 8)
    planes = []
    for c in range(plan.comps):
        q = plan.quant[plan.tq[c]].astype(np.int64).reshape(8, 8)
        if c == 0 and plan.comps == 3:
            b = blocks[:, :, :ny].reshape(my, mx, plan.vs, plan.hs, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * plan.vs, mx * plan.hs, 8, 8)
        else:
            b = blocks[:, :, ny + c - 1 if plan.comps == 3 else 0]
        s = _idct_pass((b * q).swapaxes(-1, -2), True).swapaxes(-1, -2)   # down the columns
        s = _idct_pass(s, False)                                           # along the rows
        s = np.clip(s + 128, 0, 255).astype(np.uint8)
        planes.append(s.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8))
    return planes


def _up_h(c: np.ndarray) -> np.ndarray:
    """h2v1 fancy upsampling of int64 [rows][cw] -> [rows][2 cw]."""
    left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    o = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
    o[:, 0], o[:, -1] = c[:, 0], c[:, -1]
    return o


def _up_hv(c: np.ndarray) -> np.ndarray:
    """h2v2 fancy upsampling of int64 [ch][cw] -> [2 ch][2 cw] (tools/degrade_folder.py:jpeg_roundtrip's)."""
    above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    cs = np.empty((2 * c.shape[0], c.shape[1]), dtype=np.int64)
    cs[0::2], cs[1::2] = 3 * c + above, 3 * c + below
    left, right = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1), np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    o = np.empty((cs.shape[0], 2 * cs.shape[1]), dtype=np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * cs + left + 8) >> 4, (3 * cs + right + 7) >> 4
    return o


def pixels_of(plan: Plan, coef: np.ndarray) -> np.ndarray:
    h, w = plan.h, plan.w
    planes = component_planes(plan, coef)
    yy = planes[0][:h, :w].astype(np.int64)
    if plan.comps == 1:
        return np.repeat(yy.astype(np.uint8)[..., None], 3, axis=2)
    ch, cw = -(-h // plan.vs), -(-w // plan.hs)
    cb, cr = (p[:ch, :cw].astype(np.int64) for p in planes[1:])
    if plan.hs == 2:
        cb, cr = ((_up_hv(c) if plan.vs == 2 else _up_h(c))[:h, :w] for c in (cb, cr))
    cb, cr = cb - 128, cr - 128
    out = np.stack([yy + ((_fix(1.402) * cr + 32768) >> 16),
                    yy + ((-_fix(.34414) * cb - _fix(.71414) * cr + 32768) >> 16),
                    yy + ((_fix(1.772) * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def decode_pixels(plan: Plan) -> np.ndarray:
    """uint8 [h][w][3]: what np.array(Image.open(f).convert("RGB")) gives."""
    return pixels_of(plan, decode_coefficients(plan))


def main():
    ap = argparse.ArgumentParser(description="decode a baseline JPEG through the definition of ir_jpeg_decode")
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?", help="where to save the pixels (PNG)")
    ap.add_argument("--compare", action="store_true", help="compare with Pillow's decode")
    ap.add_argument("--parallel", type=int, default=0, metavar="BITS", help="also run the parallel entropy model at this subsequence size")
    args = ap.parse_args()
    plan, why = parse(Path(args.src).read_bytes())
    if plan is None:
        print(f"{args.src}: not taken ({why})")
        return 2
    px = decode_pixels(plan)
    print(f"{args.src}: {plan.w} x {plan.h}, {plan.comps} component(s), luma {plan.hs}x{plan.vs}, restart {plan.restart}, {len(plan.scan)} scan bytes")
    if args.parallel:
        coef, rounds = parallel_entropy_model(plan, args.parallel)
        print(f"parallel model at {args.parallel} bits: {rounds} rounds, coefficients {'equal' if np.array_equal(coef, decode_coefficients(plan)) else 'DIFFER'}")
    from PIL import Image
    if args.compare:
        ref = np.array(Image.open(args.src).convert("RGB"))
        same = np.array_equal(ref, px)
        print("equal to Pillow" if same else f"DIFFERS from Pillow in {int(np.count_nonzero(ref != px))} bytes")
        if not same:
            return 1
    if args.dst:
        Image.fromarray(px).save(args.dst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
