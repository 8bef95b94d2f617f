// Baseline JPEG files into uint8 HWC RGB device images (ir_jpeg_decode): the definition of tools/jpeg_decode_model.py, whose pixels are Pillow's.
// The host has parsed the markers and removed the byte stuffing; one file is a chain of launches on the stream (the files of a batch follow
// each other through one workspace). A baseline scan is one serial bit stream per restart interval, so the entropy decode is the
// self-synchronising one of Weissenberger & Schmidt ("Massively Parallel Huffman Decoding on GPUs", ICPP 2018), arranged so that the RESULT never
// depends on how fast a stream synchronises and the number of launches never depends on the data:
//   prep     the interval table made safe (offsets and bit counts clamped into the stream) and the first subsequence of every interval: a
//            subsequence is subseq_bits bits of ONE interval, so the first of an interval starts in a known state (block 0, coefficient 0).
//   round    x SYNC_ROUNDS, one lane per subsequence: the entry state is the left neighbour's exit state of the round before (round 0: the guess
//            "a block of component 0 starts at my first bit"); a lane whose entry state did not change keeps its exit state without decoding.
//            A state is (bit position, block of the MCU, coefficient index); photographs settle within 6 rounds at 1024 bits.
//   finish   one workgroup per interval repeats the same round over the interval's subsequences until no entry state changes. By induction
//            over the subsequences that fixed point is the sequential decode, whatever the rounds before left behind; streams that do not
//            synchronise (noise at quality 100: blocks end by counting to 64, nothing re-aligns the coefficient index) cost up to one round per
//            subsequence here - slow, bounded, right. Then the exclusive scan of the blocks finished per subsequence and the interval's
//            check (end state, block count).
//   write    every subsequence again from its entry state, now storing DC differences and AC values into the zero-filled [block][64]; these
//            are the true states, so a symbol that cannot be decoded here is the file's error (decode_sub).
//   dc       one workgroup per interval and component: the prefix sum of the DC differences.
//   idct     eight lanes per block (degrade.hip's arrangement): dequantise, jidctint.c down the columns and along the rows, + 128, clamp, into
//            the component's plane.
//   rgb      one lane per output pixel: fancy upsampling on the true chroma size, YCbCr -> RGB, the crop to h x w; lane 0 writes info.
// No kernel waits for another workgroup, every loop is bounded by its interval's bit count or subsequence count, every read of the stream by
// the interval's (clamped) bit count.
#include <algorithm>

#include "../../include/instarevive_hip.h"
#include "common.h"
#include "jpeg_back.h"
#include "kernels.h"

namespace {

using namespace ir_jpeg_back;

constexpr int TPB = 256;
constexpr int SYNC_ROUNDS = 8;
enum { E_CODE = 1, E_INDEX = 2, E_PAST = 3, E_COUNT = 4 };

// the table blob of jpeg_decode.py (IR_JPEG_DECODE_TABLE_BYTES); Huffman tables in the order DC 0, DC 1, AC 0, AC 1
struct Tables {
    uint16_t lut[4][512];    // by the next 9 bits: length << 8 | symbol, 0 for a code longer than 9 bits
    uint32_t limit[4][17];   // [l]: one past the last code of at most l bits, left-aligned in 16 bits
    int32_t valoff[4][17];   // [l]: index of the first symbol of length l minus its first code
    uint8_t vals[4][256];    // symbols in code order
    uint16_t quant[4][64];   // natural order
};
static_assert(sizeof(Tables) == IR_JPEG_DECODE_TABLE_BYTES, "the blob's layout is shared with jpeg_decode.py");

struct State {
    uint32_t p, bk;   // bit position in the interval; block of the MCU | coefficient index << 8
};
IR_DEVINL bool same(State a, State b) { return a.p == b.p && a.bk == b.bk; }

// everything a kernel needs about one file
struct File {
    const uint32_t* words;   // the stream
    const uint32_t* intervals;
    const Tables* tables;
    uint32_t stream_words;
    int n_intervals, h, w, comps, hs, vs, restart, mcux, mcus, bpm, S;
    uint8_t tq[4], td[4], ta[4];
    // workspace
    uint2* iv;            // [n_intervals] clamped word offset, bit count
    uint32_t* sub_first;  // [n_intervals + 1]
    State *entry, *out[2];   // [sub_cap]
    uint32_t *cnt, *first;   // [sub_cap] blocks finished in the subsequence; blocks finished in front of it in its interval
    unsigned long long* err;   // the least (interval << 32 | subsequence << 3 | error class) of the file, all ones without an error
    int16_t* coef;
    uint8_t* planes;
    uint32_t sub_cap;
};

__constant__ uint8_t NATURAL[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

IR_DEVINL int mcus_of(const File& f, int j) {   // MCUs of interval j
    if (f.restart <= 0) return f.mcus;
    const long left = (long)f.mcus - (long)j * f.restart;
    return left < f.restart ? (left > 0 ? (int)left : 0) : f.restart;
}
IR_DEVINL int comp_of(const File& f, int b) { return f.comps == 1 ? 0 : (b < f.hs * f.vs ? 0 : b - f.hs * f.vs + 1); }

// The interval's bits through a 64-bit window in registers: words[at] above words[at + 1], big-endian. A decoder moves forward by less than 32
// bits per symbol, so a peek loads one new word per 32 bits of stream instead of two per symbol. Words past the interval read as zero.
struct BitReader {
    const uint32_t* __restrict__ words;
    uint32_t nw, at;
    uint64_t win;
    IR_DEVINL uint32_t word(uint32_t i) const { return i < nw ? __builtin_bswap32(words[i]) : 0u; }
    IR_DEVINL void seek(uint32_t p) {
        at = p >> 5;
        win = ((uint64_t)word(at) << 32) | word(at + 1);
    }
    IR_DEVINL uint32_t peek(uint32_t p) {   // the 32 bits from bit p on
        const uint32_t w = p >> 5;
        if (w == at + 1) {
            win = (win << 32) | word(w + 1);
            at = w;
        } else if (w != at) {
            seek(p);
        }
        return (uint32_t)((win << (p & 31)) >> 32);
    }
};

// Decode from state s up to the first symbol boundary at or behind `end` (<= bits). Returns the exit state; nblk = blocks finished. WRITE: the
// values go to coef[blk ..][64] for blocks below blk_end (blk: the block s stands in). A symbol that cannot be decoded ends the subsequence in
// the state its right neighbour guesses, (end, block 0, coefficient 0), with err = the error class: a guess that went wrong is nobody's
// error and must not keep the subsequences to its right from synchronising, so only the write pass, which walks the true states, reports err.
template <bool WRITE>
IR_DEVINL State decode_sub(const File& f, const Tables& T, const uint32_t* __restrict__ words, uint32_t bits, uint32_t end, State s, uint32_t& nblk,
                           uint32_t& err, long blk, long blk_end) {
    nblk = 0, err = 0;
    uint32_t p = s.p;
    int b = (int)(s.bk & 255), k = (int)(s.bk >> 8);
    const State resync{end, 0};
    if (b >= f.bpm || k > 63) {   // no state the kernels write
        err = E_INDEX;
        return resync;
    }
    BitReader br{words, (bits + 31) >> 5, 0, 0};
    if (p < end) br.seek(p);
    while (p < end) {
        if (k == 0 && b == 0 && bits - p < 8) {   // behind the last MCU the byte is padded with 1-bits
            const uint32_t rem = bits - p;
            if ((br.peek(p) >> (32 - rem)) == (1u << rem) - 1u) {
                p = bits;
                break;
            }
        }
        const int comp = comp_of(f, b), t = k == 0 ? f.td[comp] : 2 + f.ta[comp];
        const uint32_t v = br.peek(p);
        int len = T.lut[t][v >> 23] >> 8, sym = T.lut[t][v >> 23] & 255;
        if (!len) {
            const uint32_t v16 = v >> 16;
            for (int l = 10; l <= 16; ++l)
                if (v16 < T.limit[t][l]) {
                    len = l;
                    break;
                }
            if (!len) { err = E_CODE; return resync; }
            sym = T.vals[t][(T.valoff[t][len] + (int)(v16 >> (16 - len))) & 255];
        }
        int size, run = 0;
        if (k == 0) {
            if (sym > 11) { err = E_CODE; return resync; }
            size = sym;
        } else {
            size = sym & 15, run = sym >> 4;
        }
        if (p + len + size > bits) { err = E_PAST; return resync; }
        int val = 0;
        if (size) {
            const uint32_t raw = (v << len) >> (32 - size);   // a code has at most 16 bits and a value at most 15: both lie in v
            val = raw < (1u << (size - 1)) ? (int)raw - (1 << size) + 1 : (int)raw;
        }
        p += len + size;
        bool done = false;
        if (k == 0) {
            if (WRITE && blk < blk_end) f.coef[blk * 64] = (int16_t)val;
            k = 1;
        } else if (size == 0) {
            if (run == 15) {
                k += 16;
                if (k > 63) { err = E_INDEX; return resync; }
            } else {
                done = true;   // EOB
            }
        } else {
            k += run;
            if (k > 63) { err = E_INDEX; return resync; }
            if (WRITE && blk < blk_end) f.coef[blk * 64 + NATURAL[k]] = (int16_t)val;
            done = ++k == 64;
        }
        if (done) {
            k = 0, b = b + 1 == f.bpm ? 0 : b + 1;
            ++nblk, ++blk;
        }
    }
    return State{p, (uint32_t)b | ((uint32_t)k << 8)};
}

IR_DEVINL void load_tables(Tables& T, const Tables* __restrict__ src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(&T);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 4); i += TPB) d[i] = s[i];
    __syncthreads();
}

// the interval of subsequence g: the last j with sub_first[j] <= g
IR_DEVINL int interval_of(const File& f, uint32_t g) {
    int lo = 0, hi = f.n_intervals - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (f.sub_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------- prep: one workgroup
__global__ __launch_bounds__(TPB) void jpeg_prep_kernel(File f) {
    __shared__ uint32_t s_scan[TPB];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0, *f.err = ~0ull;
    __syncthreads();
    for (int base = 0; base < f.n_intervals; base += TPB) {
        const int j = base + threadIdx.x;
        uint32_t subs = 0;
        if (j < f.n_intervals) {
            uint32_t off = f.intervals[2 * j] >> 2, bits = f.intervals[2 * j + 1];
            if (off > f.stream_words) off = f.stream_words;
            const uint64_t room = (uint64_t)(f.stream_words - off) * 32;
            if (bits > room) bits = (uint32_t)room;
            if (bits > 0xfffffff0u - (uint32_t)f.S) bits = 0xfffffff0u - (uint32_t)f.S;   // positions and ends stay inside 32 bits
            f.iv[j] = make_uint2(off, bits);
            subs = (bits + (uint32_t)f.S - 1) / (uint32_t)f.S;
            if (subs < 1) subs = 1;   // an empty interval still reports its missing blocks
        }
        s_scan[threadIdx.x] = subs;
        __syncthreads();
        for (int o = 1; o < TPB; o <<= 1) {
            const uint32_t add = (int)threadIdx.x >= o ? s_scan[threadIdx.x - o] : 0;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        const uint64_t at = (uint64_t)s_carry + s_scan[threadIdx.x] - subs;   // exclusive
        if (j < f.n_intervals) f.sub_first[j] = at < f.sub_cap ? (uint32_t)at : f.sub_cap;
        __syncthreads();
        if (threadIdx.x == TPB - 1) {
            const uint64_t c = (uint64_t)s_carry + s_scan[TPB - 1];
            s_carry = c < f.sub_cap ? (uint32_t)c : f.sub_cap;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) f.sub_first[f.n_intervals] = s_carry;
}

// ---------------------------------------------------------------- round r: one lane per subsequence
__global__ __launch_bounds__(TPB) void jpeg_round_kernel(File f, int r) {
    __shared__ Tables T;
    load_tables(T, f.tables);
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    if (g >= f.sub_first[f.n_intervals]) return;
    const int j = interval_of(f, g);
    const uint32_t l = g - f.sub_first[j], bits = f.iv[j].y, S = (uint32_t)f.S;
    const uint32_t start = l * S < bits ? l * S : bits, end = bits - start > S ? start + S : bits;
    const State* prev = f.out[(r + 1) & 1];
    State* next = f.out[r & 1];
    const State e = l == 0 ? State{0, 0} : (r == 0 ? State{start, 0} : prev[g - 1]);
    if (r > 0 && same(e, f.entry[g])) {
        next[g] = prev[g];
        return;
    }
    f.entry[g] = e;
    uint32_t nblk, err;
    next[g] = decode_sub<false>(f, T, f.words + f.iv[j].x, bits, end, e, nblk, err, 0, 0);
    f.cnt[g] = nblk;
}

// ---------------------------------------------------------------- finish: one workgroup per interval
__global__ __launch_bounds__(TPB) void jpeg_finish_kernel(File f) {
    __shared__ Tables T;
    __shared__ uint32_t s_scan[TPB];
    __shared__ uint32_t s_carry;
    load_tables(T, f.tables);
    const int j = blockIdx.x;
    const uint32_t g0 = f.sub_first[j], count = f.sub_first[j + 1] - g0, bits = f.iv[j].y, S = (uint32_t)f.S;
    State* out = f.out[(SYNC_ROUNDS - 1) & 1];
    const uint32_t* words = f.words + f.iv[j].x;
    for (uint32_t round = 0; round <= count; ++round) {   // at most one round per subsequence: round r settles subsequence r
        int dirty = 0;
        for (uint32_t l = 1 + threadIdx.x; l < count; l += TPB) {
            const State e = out[g0 + l - 1];
            const bool d = !same(e, f.entry[g0 + l]);
            f.entry[g0 + l] = e;
            f.cnt[g0 + l] = d ? f.cnt[g0 + l] | 0x80000000u : f.cnt[g0 + l];   // the top bit marks "decode me" for the second phase
            dirty |= d;
        }
        if (!__syncthreads_or(dirty)) break;
        for (uint32_t l = 1 + threadIdx.x; l < count; l += TPB) {
            if (!(f.cnt[g0 + l] & 0x80000000u)) continue;
            const uint32_t start = l * S < bits ? l * S : bits, end = bits - start > S ? start + S : bits;
            uint32_t nblk, err;
            out[g0 + l] = decode_sub<false>(f, T, words, bits, end, f.entry[g0 + l], nblk, err, 0, 0);
            f.cnt[g0 + l] = nblk;
        }
        __syncthreads();
    }
    // exclusive scan of the blocks finished per subsequence
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < count; base += TPB) {
        const uint32_t l = base + threadIdx.x, c = l < count ? f.cnt[g0 + l] & 0x7fffffffu : 0;
        s_scan[threadIdx.x] = c;
        __syncthreads();
        for (int o = 1; o < TPB; o <<= 1) {
            const uint32_t add = (int)threadIdx.x >= o ? s_scan[threadIdx.x - o] : 0;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (l < count) f.first[g0 + l] = s_carry + s_scan[threadIdx.x] - c;
        __syncthreads();
        if (threadIdx.x == TPB - 1) s_carry += s_scan[TPB - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t want = (uint32_t)mcus_of(f, j) * (uint32_t)f.bpm;
        bool bad = count == 0;   // the subsequence grid ran out (an interval table that overlaps itself)
        if (!bad) {
            const State last = out[g0 + count - 1];
            bad = last.p != bits || last.bk != 0 || s_carry != want;
        }
        if (bad) atomicMin(f.err, ((unsigned long long)j << 32) | (0x1fffffffull << 3) | E_COUNT);   // behind every decode error of the interval
    }
}

// ---------------------------------------------------------------- write: one lane per subsequence
__global__ __launch_bounds__(TPB) void jpeg_write_kernel(File f) {
    __shared__ Tables T;
    load_tables(T, f.tables);
    const uint32_t g = blockIdx.x * TPB + threadIdx.x;
    if (g >= f.sub_first[f.n_intervals]) return;
    const int j = interval_of(f, g);
    const uint32_t l = g - f.sub_first[j], bits = f.iv[j].y, S = (uint32_t)f.S;
    const uint32_t start = l * S < bits ? l * S : bits, end = bits - start > S ? start + S : bits;
    const long base = (long)j * (f.restart > 0 ? f.restart : 0) * f.bpm, blk_end = base + (long)mcus_of(f, j) * f.bpm;
    uint32_t nblk, err;
    decode_sub<true>(f, T, f.words + f.iv[j].x, bits, end, f.entry[g], nblk, err, base + f.first[g], blk_end);
    if (err) atomicMin(f.err, ((unsigned long long)j << 32) | ((unsigned long long)l << 3) | err);
}

// ---------------------------------------------------------------- dc: one workgroup per (interval, component)
__global__ __launch_bounds__(TPB) void jpeg_dc_kernel(File f) {
    __shared__ int s_scan[TPB];
    const int j = blockIdx.x, c = blockIdx.y;
    const int nb = f.comps == 1 || c > 0 ? 1 : f.hs * f.vs, o = f.comps == 1 || c == 0 ? 0 : f.hs * f.vs + c - 1;   // blocks per MCU, first of them
    const long base = (long)j * (f.restart > 0 ? f.restart : 0) * f.bpm;
    const int len = mcus_of(f, j) * nb, chunk = (len + TPB - 1) / TPB;
    const int i0 = min((int)threadIdx.x * chunk, len), i1 = min(i0 + chunk, len);
    auto at = [&](int i) -> int16_t& { return f.coef[(base + (long)(i / nb) * f.bpm + o + i % nb) * 64]; };
    int sum = 0;
    for (int i = i0; i < i1; ++i) sum += at(i);
    s_scan[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 1; k < TPB; k <<= 1) {
        const int add = (int)threadIdx.x >= k ? s_scan[threadIdx.x - k] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    int run = s_scan[threadIdx.x] - sum;
    for (int i = i0; i < i1; ++i) {
        run += at(i);
        at(i) = (int16_t)run;
    }
}

// ---------------------------------------------------------------- idct: eight lanes per block
IR_DEVINL int plane_w(const File& f, int c) { return f.mcux * 8 * (c == 0 && f.comps == 3 ? f.hs : 1); }
IR_DEVINL int plane_h(const File& f, int c) { return (f.mcus / f.mcux) * 8 * (c == 0 && f.comps == 3 ? f.vs : 1); }
IR_DEVINL uint8_t* plane_of(const File& f, int c) {
    uint8_t* p = f.planes;
    for (int i = 0; i < c; ++i) p += (size_t)plane_w(f, i) * plane_h(f, i);
    return p;
}

__global__ __launch_bounds__(TPB) void jpeg_idct_kernel(File f) {
    __shared__ int s_c[TPB / 8][8][9];
    const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
    const long nblk = (long)f.mcus * f.bpm, blk = (long)blockIdx.x * (TPB / 8) + g;
    const bool live = blk < nblk;
    i64 d[8];
    uint8_t* row = nullptr;
    if (live) {
        const int m = (int)(blk / f.bpm), b = (int)(blk - (long)m * f.bpm), c = comp_of(f, b);
        const int my = m / f.mcux, mx = m - my * f.mcux;
        const int bx = c == 0 && f.comps == 3 ? mx * f.hs + b % f.hs : mx, by = c == 0 && f.comps == 3 ? my * f.vs + b / f.hs : my;
        row = plane_of(f, c) + (size_t)(by * 8 + l) * plane_w(f, c) + bx * 8;
        const int16_t* co = f.coef + blk * 64;
        const uint16_t* q = f.tables->quant[f.tq[c]];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (i64)co[i * 8 + l] * q[i * 8 + l];   // column l
        idct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_c[g][i][l] = (int)d[i];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_c[g][l][i];
        idct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = (uint8_t)clampi((int)d[i] + 128, 0, 255);
    }
}

// ---------------------------------------------------------------- rgb: one lane per output pixel
__global__ __launch_bounds__(TPB) void jpeg_rgb_kernel(File f, uint8_t* __restrict__ out, long pitch, uint32_t* __restrict__ info) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i == 0) {
        const unsigned long long e = *f.err;
        *info = e == ~0ull ? 0u : (uint32_t)(e & 7u);
    }
    if (i >= (long)f.h * f.w) return;
    const int y = (int)(i / f.w), x = (int)(i - (long)y * f.w);
    const int YW = plane_w(f, 0);
    const uint8_t* Y = f.planes;
    const int yy = Y[(size_t)y * YW + x];
    uint8_t* o = out + (long)y * pitch + 3L * x;
    if (f.comps == 1) {
        o[0] = o[1] = o[2] = (uint8_t)yy;
        return;
    }
    const int CW = plane_w(f, 1);
    const uint8_t *Cb = plane_of(f, 1), *Cr = plane_of(f, 2);
    int cb, cr;
    if (f.hs == 1) {
        cb = Cb[(size_t)y * CW + x], cr = Cr[(size_t)y * CW + x];
    } else if (f.vs == 1) {
        const int cw = (f.w + 1) >> 1;
        cb = chroma_up_h(Cb + (size_t)y * CW, cw, x), cr = chroma_up_h(Cr + (size_t)y * CW, cw, x);
    } else {
        const int ch = (f.h + 1) >> 1, cw = (f.w + 1) >> 1;
        cb = chroma_up(Cb, CW, ch, cw, y, x), cr = chroma_up(Cr, CW, ch, cw, y, x);
    }
    cb -= 128, cr -= 128;
    o[0] = (uint8_t)clampi(yy + ((FIX(1.402) * cr + 32768) >> 16), 0, 255);
    o[1] = (uint8_t)clampi(yy + ((-FIX(.34414) * cb - FIX(.71414) * cr + 32768) >> 16), 0, 255);
    o[2] = (uint8_t)clampi(yy + ((FIX(1.772) * cb + 32768) >> 16), 0, 255);
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t iv, sub_first, entry, out0, out1, cnt, first, err, coef, planes, total;
    uint32_t sub_cap;
};

// One formula for every sampling and restart interval: the block count of 4:4:4 on the 16-pixel grid (no sampling taken has more), at most one
// interval per MCU, and per interval one subsequence more than its bits fill.
Layout layout(int h, int w, uint32_t stream_bytes, int S) {
    const size_t blocks = 12 * (size_t)((h + 15) / 16) * ((w + 15) / 16), intervals = blocks;
    Layout l;
    l.sub_cap = (uint32_t)std::min<size_t>(((size_t)stream_bytes * 8) / S + intervals + 1, 0x7fffffff);
    size_t at = 0;
    l.iv = at, at += up256(intervals * 8);
    l.sub_first = at, at += up256((intervals + 1) * 4);
    l.entry = at, at += up256((size_t)l.sub_cap * 8);
    l.out0 = at, at += up256((size_t)l.sub_cap * 8);
    l.out1 = at, at += up256((size_t)l.sub_cap * 8);
    l.cnt = at, at += up256((size_t)l.sub_cap * 4);
    l.first = at, at += up256((size_t)l.sub_cap * 4);
    l.err = at, at += 256;
    l.coef = at, at += up256(blocks * 128);
    l.planes = at, at += up256(blocks * 64);
    l.total = at;
    return l;
}

struct Geometry {
    int mcux, mcuy, bpm;
};
Geometry geometry(const ir_jpeg_file* f) {
    const int mw = 8 * (f->comps == 3 ? f->hs : 1), mh = 8 * (f->comps == 3 ? f->vs : 1);
    return Geometry{(f->w + mw - 1) / mw, (f->h + mh - 1) / mh, f->comps == 3 ? f->hs * f->vs + 2 : 1};
}

}  // namespace

int ir_jpeg_decode_check(const ir_jpeg_file* f, const char** why) {
    auto bad = [why](const char* w) { *why = w; return -1; };
    if (!f->stream || !f->intervals || !f->tables || !f->out) return bad("null pointer in the record");
    if (f->h < 8 || f->w < 8 || f->h > 65535 || f->w > 65535) return bad("sides outside 8 .. 65535");
    if (f->pitch < 3L * f->w) return bad("pitch below 3 w");
    if (f->comps != 1 && f->comps != 3) return bad("components other than 1 or 3");
    if (f->comps == 1 ? (f->hs != 1 || f->vs != 1) : !((f->hs == 1 && f->vs == 1) || (f->hs == 2 && (f->vs == 1 || f->vs == 2))))
        return bad("luma sampling other than 1 x 1, 2 x 1, 2 x 2");
    for (int c = 0; c < f->comps; ++c)
        if (f->tq[c] > 3 || f->td[c] > 1 || f->ta[c] > 1) return bad("table number outside 0 .. 3 (quantisation) or 0 .. 1 (Huffman)");
    if (f->restart_mcus < 0 || f->restart_mcus > 65535) return bad("restart interval outside 0 .. 65535");
    const Geometry g = geometry(f);
    const long mcus = (long)g.mcux * g.mcuy, want = f->restart_mcus ? (mcus + f->restart_mcus - 1) / f->restart_mcus : 1;
    if (f->n_intervals != want) return bad("n_intervals is not ceil(MCUs / restart_mcus)");
    if (f->stream_bytes < 4 || (f->stream_bytes & 3) || f->stream_bytes > 0x7ffffff0u) return bad("stream_bytes no multiple of 4 in 4 .. 2^31");
    if ((reinterpret_cast<uintptr_t>(f->stream) & 3) || (reinterpret_cast<uintptr_t>(f->intervals) & 3) || (reinterpret_cast<uintptr_t>(f->tables) & 3))
        return bad("misaligned stream, interval table or tables");
    return 0;
}

long ir_jpeg_decode_blocks(const ir_jpeg_file* f) {
    const Geometry g = geometry(f);
    return (long)g.mcux * g.mcuy * g.bpm;
}

size_t ir_jpeg_decode_workspace(int h, int w, uint32_t stream_bytes, int subseq_bits) {
    if (h < 8 || w < 8 || h > 65535 || w > 65535 || subseq_bits < 128 || subseq_bits > 4096 || subseq_bits % 32 || stream_bytes > 0x7ffffff0u) return 0;
    return layout(h, w, stream_bytes, subseq_bits).total;
}

int ir_launch_jpeg_decode(const ir_jpeg_file* r, int subseq_bits, uint32_t* info, int16_t* coef, void* ws, hipStream_t s) {
    const char* why;
    if (ir_jpeg_decode_check(r, &why) || subseq_bits < 128 || subseq_bits > 4096 || subseq_bits % 32) return -1;
    const Layout l = layout(r->h, r->w, r->stream_bytes, subseq_bits);
    const Geometry g = geometry(r);
    uint8_t* b = static_cast<uint8_t*>(ws);
    File f;
    f.words = reinterpret_cast<const uint32_t*>(r->stream);
    f.intervals = r->intervals;
    f.tables = static_cast<const Tables*>(r->tables);
    f.stream_words = r->stream_bytes / 4;
    f.n_intervals = r->n_intervals, f.h = r->h, f.w = r->w, f.comps = r->comps, f.hs = r->hs, f.vs = r->vs, f.restart = r->restart_mcus;
    f.mcux = g.mcux, f.mcus = g.mcux * g.mcuy, f.bpm = g.bpm, f.S = subseq_bits;
    for (int c = 0; c < 4; ++c) f.tq[c] = r->tq[c], f.td[c] = r->td[c], f.ta[c] = r->ta[c];
    f.iv = reinterpret_cast<uint2*>(b + l.iv);
    f.sub_first = reinterpret_cast<uint32_t*>(b + l.sub_first);
    f.entry = reinterpret_cast<State*>(b + l.entry);
    f.out[0] = reinterpret_cast<State*>(b + l.out0), f.out[1] = reinterpret_cast<State*>(b + l.out1);
    f.cnt = reinterpret_cast<uint32_t*>(b + l.cnt), f.first = reinterpret_cast<uint32_t*>(b + l.first);
    f.err = reinterpret_cast<unsigned long long*>(b + l.err);
    f.coef = coef ? coef : reinterpret_cast<int16_t*>(b + l.coef);
    f.planes = b + l.planes;
    const long blocks = (long)f.mcus * f.bpm;
    // the most subsequences the file can have: the launches are sized by it, never by what the stream says, and prep lets no interval table ask for more
    const size_t subs = std::min<size_t>(((size_t)r->stream_bytes * 8) / subseq_bits + (size_t)r->n_intervals + 1, l.sub_cap);
    f.sub_cap = (uint32_t)subs;
    const dim3 sub_grid((unsigned)((subs + TPB - 1) / TPB));
    if (hipMemsetAsync(f.coef, 0, (size_t)blocks * 128, s) != hipSuccess) return -1;
    hipLaunchKernelGGL(jpeg_prep_kernel, dim3(1), dim3(TPB), 0, s, f);
    for (int k = 0; k < SYNC_ROUNDS; ++k) hipLaunchKernelGGL(jpeg_round_kernel, sub_grid, dim3(TPB), 0, s, f, k);
    hipLaunchKernelGGL(jpeg_finish_kernel, dim3(f.n_intervals), dim3(TPB), 0, s, f);
    hipLaunchKernelGGL(jpeg_write_kernel, sub_grid, dim3(TPB), 0, s, f);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(f.n_intervals, f.comps), dim3(TPB), 0, s, f);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + TPB / 8 - 1) / (TPB / 8))), dim3(TPB), 0, s, f);
    hipLaunchKernelGGL(jpeg_rgb_kernel, dim3((unsigned)(((long)r->h * r->w + TPB - 1) / TPB)), dim3(TPB), 0, s, f, r->out, r->pitch, info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
