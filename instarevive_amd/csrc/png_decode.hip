// PNG decoding on the device (ir_png_decode): a zlib stream (RFC 1950 / 1951) to the inflated bytes, the PNG unfilter, HWC RGB8. The pixels are
// Pillow's, np.array(Image.open(f).convert("RGB")), byte for byte; tools/png_decode_model.py states every phase in numpy and is what the tables
// this file leaves in the workspace are tested against. The contract and the workspace's sections: include/instarevive_hip.h.
//
// Inflate is serial: a block's position in the stream and in the output is known only once everything before it is decoded. What makes it
// parallel here is that a dynamic-Huffman block starts with a header that can be recognised at any bit offset (find_kernel), that a decoder
// started at such an offset needs no history to COUNT its output (size_kernel), and that a copy can be recorded as a pointer and followed later
// (write_kernel, round_kernel). Ordering comes from kernel boundaries alone: no workgroup waits for another, no flag is spun on.
//
//   find    one lane per bit offset: BTYPE = 2, HLIT <= 29, HDIST <= 29 and a complete code-length code (about 1 offset in 1000 passes), then the
//           full header parse on the survivors - code lengths that parse without overrun, symbol 256 present, literal and distance codes complete
//           by zlib's rule (inftrees.c: over-subscribed never, incomplete only as a single code of length 1, or no distance code at all).
//           atomicMin keeps the first candidate of every span of span_bits bits. A false candidate costs time only: chain_kernel never reaches it.
//   size    one wave per entry (bit 16, and every span's candidate): all 64 lanes run the same decode, so its state lives in scalar registers and
//           the tables in LDS; it walks blocks of any type and stops at the first block end that is the candidate recorded for the span the end
//           lies in, at BFINAL, or at an error.
//   chain   one lane follows the entries from bit 16, gives each its output offset and checks the total against h (1 + w bpp).
//   write   the chain's entries again: lane 0 writes a literal byte i with src[i] = i, the lanes share a match (src[i] = i - distance) and a
//           stored block. A distance that reaches before the output's start is error 4 and the byte points at itself.
//   round   src[i] = src[src[i]], ceil(log2(bytes)) times, IN PLACE. That is correct: src[i] <= i always, and at any moment every src[j] is an
//           ancestor of j on j's chain of copies that is at least as far as the round's start value, whichever of a concurrent reader and writer
//           comes first (an aligned 32-bit store is not torn) - so a round at least halves every chain's depth, as the double-buffered form does,
//           and a round that changes nothing has found every root. A round returns at once when the round before set no flag.
//   gather  byte[i] = literal[src[i]]; adler  per 16 KB the two sums, then one lane joins them and compares with the trailer.
//   unfilter  one workgroup of 1024 lanes, lane = row, skewed by one group of 4 pixels: lane r reads the group above from the LDS slot lane r - 1
//           filled one step earlier, so Paeth's left / up / up-left are all at hand and an all-Paeth image costs what any other does. Rows
//           beyond 1024 are taken by the same lanes in turn, without draining the skew: lane 0 reads its row above from the unfiltered bytes in
//           global memory, which lane 1023 wrote at least one barrier earlier. Steps: (ceil(h / 1024) - 1) max(ceil(w / 4), 1024) + 1023 + ceil(w / 4).
//   rgb     grey replicated, alpha dropped, into out at pitch; info.
//
// Worst case: a stream with no dynamic block (stored or fixed-Huffman blocks alone) has one entry, and size and write are one wave's serial walk
// of the whole stream - the host refuses such files above 64 KB when they begin with a fixed block (png_decode.py: "fixed"). Every loop is bounded
// by the stream's bit count (a symbol takes at least one bit) or by the expected size (a count above it ends the walk with error 6).
//
// Measured on one MI355X (profiles/png_decoder.txt), a photograph-like 2048 x 2048 file at Pillow's default level, 355 blocks: find 0.74, size 4.65,
// chain 0.13, write 4.59, resolve 0.38, adler 0.18, unfilter 3.62, rgb 0.01 ms. size and write are bound by ONE wave's walk of its block - about
// 33 000 symbols at some 140 ns each - whatever the file's size (a 512 x 512 file: 4.0 and 4.5 ms); before the 64-lane literal runs a symbol
// cost 220 ns, and before the register-held stream window 320 ns. A level-1 file (120 longer blocks, short matches everywhere) takes 49 ms.
// The unfilter is bound by one CU's VALU rate: 12.6 M bytes at about 20 operations each. Splitting a block's symbols among lanes, as
// jpeg_decode.hip splits a scan, is the step that would move size and write.
#include <algorithm>
#include <type_traits>

#include "../../include/instarevive_hip.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TPB = 256;
constexpr uint32_t NONE = 0xffffffffu;
constexpr int FIND_RUN = 4096;   // bit offsets per find workgroup (one wave): 64 steps of 64 lanes
constexpr int LUT_BITS = 10;
enum { E_HEADER = 1, E_CODE = 2, E_PAST = 3, E_DIST = 4, E_STORED = 5, E_SIZE = 6, E_ADLER = 7, E_FILTER = 8 };

struct File {
    const uint32_t* words;
    uint32_t nwords, nbits, span, spans, entries, N, adler;
    int h, w, bpp, rb, ppitch;
    uint32_t *hdr, *cand, *e_end, *e_next, *e_len, *e_status, *e_off, *chain, *asum, *src;
    uint8_t *lit, *bytes, *pix;
};

__device__ const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__device__ const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

// 32 bits of the stream from bit `pos` on (LSB first); bits behind the stream read as zero. Any lane, any position: two loads.
__device__ __forceinline__ uint32_t peek_any(const File& f, uint32_t pos) {
    const uint32_t i = pos >> 5;
    const uint32_t lo = i < f.nwords ? f.words[i] : 0u, hi = i + 1 < f.nwords ? f.words[i + 1] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (pos & 31));
}

// The same for a whole wave that reads one position: the 64 lanes hold 64 consecutive words of the stream, a peek is two v_readlane, and memory is
// touched once per 1952 bits - a walk's symbols then wait for LDS alone, not for a load.
struct Reader {
    uint32_t v = 0, base = 0x80000000u;   // no window yet: any position refills
    __device__ __forceinline__ uint32_t window(const File& f, uint32_t pos) {   // the word of `pos` as a lane number, with three more words behind it
        const uint32_t i = pos >> 5;
        uint32_t rel = i - base;
        if (rel >= 61) {
            base = i, rel = 0;
            const uint32_t at = i + (threadIdx.x & 63);
            v = at < f.nwords ? f.words[at] : 0u;
        }
        return rel;
    }
    __device__ __forceinline__ uint32_t peek(const File& f, uint32_t pos) {
        const uint32_t rel = window(f, pos);
        const uint32_t lo = __builtin_amdgcn_readlane(v, rel), hi = __builtin_amdgcn_readlane(v, rel + 1);
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (pos & 31));
    }
    // lane l's 32 bits from bit pos + l on: 64 peeks at once
    __device__ __forceinline__ uint32_t peek_lanes(const File& f, uint32_t pos, int lane) {
        const uint32_t rel = window(f, pos);
        const uint32_t w0 = __builtin_amdgcn_readlane(v, rel), w1 = __builtin_amdgcn_readlane(v, rel + 1), w2 = __builtin_amdgcn_readlane(v, rel + 2),
                       w3 = __builtin_amdgcn_readlane(v, rel + 3);
        const uint32_t sh = (pos & 31) + lane, wi = sh >> 5;   // 0 .. 94: word 0, 1 or 2
        const uint32_t lo = wi == 0 ? w0 : wi == 1 ? w1 : w2, hi = wi == 0 ? w1 : wi == 1 ? w2 : w3;
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31));
    }
};

struct Tables {   // one wave's, in LDS
    uint16_t lut_l[1 << LUT_BITS], lut_d[1 << LUT_BITS];   // symbol | length << 9 by the next 10 bits; 0: longer than 10 bits, or no code
    uint16_t cnt_l[16], cnt_d[16], offs[16];                // codes per length (puff's count[]), and the sort's cursor
    uint16_t sym_l[288], sym_d[32];                         // symbols in canonical order
    uint8_t lens[320];
    uint8_t cl_lut[128];                                    // the code-length code: symbol | length << 5 by the next 7 bits
};

// The header of a dynamic block behind its three type bits. 0, or the error class. STORE: the lengths go to t.lens (lane 0 writes), nlen / ndist say how many.
template <bool STORE>
__device__ int parse_dynamic(const File& f, Reader& rd, uint32_t& pos, Tables& t, int lane, int& nlen, int& ndist) {
    uint32_t v = rd.peek(f, pos);
    nlen = (v & 31) + 257, ndist = ((v >> 5) & 31) + 1;
    const int ncl = ((v >> 10) & 15) + 4;
    pos += 14;
    if (nlen > 286 || ndist > 30) return E_HEADER;
    uint64_t packed = 0;
    int kraft = 0;
    for (int i = 0; i < ncl; ++i) {
        const uint32_t l = rd.peek(f, pos) & 7;
        pos += 3;
        packed |= (uint64_t)l << (3 * CL_ORDER[i]);
        if (l) kraft += 128 >> l;
    }
    if (pos > f.nbits) return E_PAST;
    if (kraft != 128) return E_HEADER;
    __syncthreads();
    if (lane == 0) {
        uint32_t code = 0;
        for (int len = 1; len <= 7; ++len) {
            for (int s = 0; s < 19; ++s)
                if (((packed >> (3 * s)) & 7) == (uint64_t)len) {
                    for (uint32_t k = __brev(code) >> (32 - len); k < 128; k += 1u << len) t.cl_lut[k] = (uint8_t)(s | (len << 5));
                    ++code;
                }
            code <<= 1;
        }
    }
    __syncthreads();
    const int total = nlen + ndist;
    int i = 0, prev = 0, kl = 0, kd = 0, maxl = 0, maxd = 0;
    bool has256 = false;
    while (i < total) {
        v = rd.peek(f, pos);
        const int e = t.cl_lut[v & 127], s = e & 31, l = e >> 5;
        int val = s, rep = 1;
        pos += l;
        if (s == 16) {
            if (i == 0) return E_HEADER;
            val = prev, rep = 3 + ((v >> l) & 3), pos += 2;
        } else if (s == 17) {
            val = 0, rep = 3 + ((v >> l) & 7), pos += 3;
        } else if (s == 18) {
            val = 0, rep = 11 + ((v >> l) & 127), pos += 7;
        }
        if (pos > f.nbits) return E_PAST;
        if (i + rep > total) return E_HEADER;
        if (STORE || val)
            for (int r = 0; r < rep; ++r) {
                const int at = i + r;
                if (STORE && lane == 0) t.lens[at] = (uint8_t)val;
                if (val) {
                    if (at < nlen) kl += 32768 >> val, maxl = max(maxl, val), has256 |= at == 256;
                    else kd += 32768 >> val, maxd = max(maxd, val);
                }
            }
        i += rep, prev = val;
    }
    if (!has256 || kl > 32768 || (kl < 32768 && maxl != 1) || kd > 32768 || (kd < 32768 && maxd > 1)) return E_HEADER;
    return 0;
}

// lens[0 .. n) to the canonical order (cnt, sym) and the 10-bit table
__device__ void build(const uint8_t* lens, int n, uint16_t* lut, uint16_t* cnt, uint16_t* sym, uint16_t* offs, int lane) {
    __syncthreads();
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) cnt[l] = 0;
        for (int s = 0; s < n; ++s) ++cnt[lens[s]];
        cnt[0] = 0;
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + cnt[l];
        for (int s = 0; s < n; ++s)
            if (lens[s]) sym[offs[lens[s]]++] = (uint16_t)s;
    }
    for (int k = lane; k < (1 << LUT_BITS); k += 64) lut[k] = 0;
    __syncthreads();
    uint32_t code = 0;
    int at = 0;
    for (int len = 1; len <= LUT_BITS; ++len) {
        const int c = cnt[len];
        for (int j = 0; j < c; ++j) {
            const uint16_t e = (uint16_t)(sym[at + j] | (len << 9));
            const uint32_t rev = __brev(code + j) >> (32 - len);
            if (rev < (1u << LUT_BITS))   // an over-subscribed code cannot come this far; the guard keeps the table's bounds whatever the lengths
                for (uint32_t k = rev + ((uint32_t)lane << len); k < (1u << LUT_BITS); k += 64u << len) lut[k] = e;
        }
        at += c, code = (code + c) << 1;
    }
    __syncthreads();
}

// one symbol by the bits v: its length in bits (0: no such code) and the symbol
__device__ __forceinline__ int decode_symbol(uint32_t v, const uint16_t* lut, const uint16_t* cnt, const uint16_t* sym, int& s) {
    const int e = lut[v & ((1 << LUT_BITS) - 1)];
    if (e >> 9) {
        s = e & 511;
        return e >> 9;
    }
    int code = 0, first = 0, at = 0;
    for (int len = 1; len <= 15; ++len) {   // puff's canonical walk
        code |= (v >> (len - 1)) & 1;
        const int c = cnt[len];
        if (code - c < first) {
            s = sym[at + (code - first)];
            return len;
        }
        at += c, first = (first + c) << 1, code <<= 1;
    }
    return 0;
}

// Walk blocks from bit `pos`. WRITE: the output offset starts at `out` and literals, stored bytes and copies are recorded, none at or behind `lim`.
// Ends at a block end that is its span's candidate (next = that entry), at BFINAL (next = NONE) or with an error; returns the error class.
template <bool WRITE>
__device__ int walk(const File& f, Tables& t, int lane, uint32_t& pos, uint32_t& out, uint32_t lim, uint32_t& next) {
    const uint32_t cap = WRITE ? lim : f.N;
    Reader rd;
    next = NONE;
    while (true) {
        if (pos + 3 > f.nbits) return E_PAST;
        uint32_t v = rd.peek(f, pos);
        const bool final = v & 1;
        const int type = (v >> 1) & 3;
        pos += 3;
        if (type == 3) return E_HEADER;
        if (type == 0) {
            pos = (pos + 7) & ~7u;
            v = rd.peek(f, pos);
            pos += 32;
            if (pos > f.nbits) return E_PAST;
            const uint32_t len = v & 0xffff;
            if ((len ^ 0xffff) != (v >> 16)) return E_STORED;
            if (len > (f.nbits - pos) / 8) return E_PAST;
            if (len > cap - out) return E_SIZE;
            if (WRITE) {
                const uint8_t* b = reinterpret_cast<const uint8_t*>(f.words) + (pos >> 3);
                for (uint32_t k = lane; k < len; k += 64) f.lit[out + k] = b[k], f.src[out + k] = out + k;
            }
            out += len, pos += 8 * len;
        } else {
            if (type == 1) {
                __syncthreads();
                if (lane == 0) {
                    for (int s = 0; s < 288; ++s) t.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
                    for (int s = 288; s < 318; ++s) t.lens[s] = 5;
                }
                build(t.lens, 288, t.lut_l, t.cnt_l, t.sym_l, t.offs, lane);
                build(t.lens + 288, 30, t.lut_d, t.cnt_d, t.sym_d, t.offs, lane);
            } else {
                int nlen, ndist;
                if (int e = parse_dynamic<true>(f, rd, pos, t, lane, nlen, ndist)) return e;
                build(t.lens, nlen, t.lut_l, t.cnt_l, t.sym_l, t.offs, lane);
                build(t.lens + nlen, ndist, t.lut_d, t.cnt_d, t.sym_d, t.offs, lane);
            }
            int hold = 0;
            while (true) {
                // A run of literals, 64 lanes at a time: lane l looks up the code at bit pos + l, then the wave follows the codes' lengths from lane
                // to lane (a v_readlane per symbol in place of a trip to LDS) while they are literals of the short table that end inside the
                // stream and inside the output. The lanes it visited write their literals side by side. Whatever ends the run - a length, the
                // end of the block, a long code, an error - is the one-symbol path's below, so the two decode alike. After an attempt that found no
                // literal the next four symbols go straight to that path: in a stretch of matches the attempt is pure cost.
                if (hold) {
                    --hold;
                } else {
                    const int e = t.lut_l[rd.peek_lanes(f, pos, lane) & ((1 << LUT_BITS) - 1)];
                    uint32_t k = 0, n = 0;
                    unsigned long long visited = 0;
                    while (k < 64 - LUT_BITS) {
                        const uint32_t ek = __builtin_amdgcn_readlane(e, k), len = ek >> 9;
                        if (!len || (ek & 511) >= 256 || pos + k + len > f.nbits || out + n >= cap) break;
                        visited |= 1ull << k, k += len, ++n;
                    }
                    if (n) {
                        if (WRITE && ((visited >> lane) & 1)) {
                            const uint32_t at = out + __popcll(visited & ((1ull << lane) - 1));
                            f.lit[at] = (uint8_t)(e & 511), f.src[at] = at;
                        }
                        out += n, pos += k;
                        continue;
                    }
                    hold = 4;
                }
                v = rd.peek(f, pos);
                int s, l = decode_symbol(v, t.lut_l, t.cnt_l, t.sym_l, s);
                if (!l) return E_CODE;
                pos += l;
                if (pos > f.nbits) return E_PAST;
                if (s < 256) {
                    if (out >= cap) return E_SIZE;
                    if (WRITE && lane == 0) f.lit[out] = (uint8_t)s, f.src[out] = out;
                    ++out;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return E_CODE;
                const uint32_t len = LEN_BASE[s - 257] + ((v >> l) & ((1u << LEN_EXTRA[s - 257]) - 1));
                pos += LEN_EXTRA[s - 257];
                v = rd.peek(f, pos);
                l = decode_symbol(v, t.lut_d, t.cnt_d, t.sym_d, s);
                if (!l || s > 29) return E_CODE;
                const uint32_t dist = DIST_BASE[s] + ((v >> l) & ((1u << DIST_EXTRA[s]) - 1));
                pos += l + DIST_EXTRA[s];
                if (pos > f.nbits) return E_PAST;
                if (len > cap - out) return E_SIZE;
                if (WRITE) {
                    const bool bad = dist > out;   // before the start of the whole output: the byte points at itself, and the file has error 4
                    for (uint32_t k = lane; k < len; k += 64) {
                        f.src[out + k] = bad ? out + k : out + k - dist;
                        if (bad) f.lit[out + k] = 0;
                    }
                    if (bad) return E_DIST;
                }
                out += len;
            }
        }
        if (final) return 0;
        const uint32_t sp = pos / f.span;
        if (sp < f.spans && f.cand[sp] == pos) {
            next = sp + 1;
            return 0;
        }
    }
}

__global__ __launch_bounds__(64) void png_find_kernel(File f) {
    __shared__ Tables t;
    const int lane = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)FIND_RUN;
    for (int step = 0; step < FIND_RUN / 64; ++step) {
        const uint32_t p = base + step * 64 + lane;
        bool ok = p >= 16 && p + 17 <= f.nbits;
        uint32_t v = 0, v2 = 0, v3 = 0;
        if (ok) {
            v = peek_any(f, p);
            ok = ((v >> 1) & 3) == 2 && ((v >> 3) & 31) <= 29 && ((v >> 8) & 31) <= 29;
        }
        if (ok) {   // the Kraft sum of the code-length code: (HCLEN + 4) fields of 3 bits behind bit 17
            v2 = peek_any(f, p + 17), v3 = peek_any(f, p + 47);
            const int ncl = ((v >> 13) & 15) + 4;
            int kraft = 0;
            for (int i = 0; i < 19; ++i) {
                const uint32_t l = i < 10 ? (v2 >> (3 * i)) & 7 : (v3 >> (3 * (i - 10))) & 7;
                if (i < ncl && l) kraft += 128 >> l;
            }
            ok = kraft == 128 && p + 17 + 3 * ncl <= f.nbits;
        }
        unsigned long long m = __ballot(ok);
        while (m) {   // the survivors, one after the other, by the whole wave
            const int who = __ffsll(m) - 1;
            m &= m - 1;
            const uint32_t p0 = base + step * 64 + who;   // below nbits, so its span exists
            uint32_t q = p0 + 3;
            int nlen, ndist;
            Reader rd;
            if (parse_dynamic<false>(f, rd, q, t, lane, nlen, ndist) == 0 && lane == 0) atomicMin(&f.cand[p0 / f.span], p0);
        }
    }
}

template <bool WRITE>
__global__ __launch_bounds__(64) void png_walk_kernel(File f) {
    __shared__ Tables t;
    const int lane = threadIdx.x;
    uint32_t e = blockIdx.x;
    if (WRITE) {
        if (f.hdr[0] || e >= f.hdr[1]) return;
        e = f.chain[e];
    }
    uint32_t pos = e == 0 ? 16u : f.cand[e - 1];
    if (pos == NONE) {
        if (lane == 0) f.e_status[e] = NONE, f.e_end[e] = NONE, f.e_next[e] = NONE, f.e_len[e] = 0;
        return;
    }
    uint32_t out = WRITE ? f.e_off[e] : 0u, next;
    const int err = walk<WRITE>(f, t, lane, pos, out, WRITE ? out + f.e_len[e] : 0u, next);
    if (lane) return;
    if (WRITE) {
        if (err) atomicCAS(&f.hdr[0], 0u, (uint32_t)err);
    } else {
        f.e_status[e] = err, f.e_end[e] = pos, f.e_next[e] = next, f.e_len[e] = out;
    }
}

__global__ void png_chain_kernel(File f) {
    if (threadIdx.x || blockIdx.x) return;
    uint32_t e = 0, off = 0, n = 0, err = 0;
    for (uint32_t it = 0; it < f.entries; ++it) {
        const uint32_t st = f.e_status[e];
        if (st) {
            err = st == NONE ? (uint32_t)E_HEADER : st;
            break;
        }
        f.chain[n++] = e, f.e_off[e] = off;
        if (f.e_len[e] > f.N - off) {
            err = E_SIZE;
            break;
        }
        off += f.e_len[e];
        const uint32_t nx = f.e_next[e];
        if (nx == NONE) break;
        if (nx <= e || nx >= f.entries) {   // cannot be: an entry ends behind its start
            err = E_HEADER;
            break;
        }
        e = nx;
    }
    if (!err && off != f.N) err = E_SIZE;
    f.hdr[0] = err, f.hdr[1] = n, f.hdr[2] = off;
}

__global__ __launch_bounds__(TPB) void png_round_kernel(File f, int r) {
    if (f.hdr[0] || (r > 0 && !f.hdr[16 + r - 1])) return;
    const uint32_t i = blockIdx.x * (uint32_t)TPB + threadIdx.x;
    bool changed = false;
    if (i < f.N) {
        const uint32_t s = min(f.src[i], i), t = min(f.src[s], s);
        if (t != s) f.src[i] = t, changed = true;
    }
    if (__ballot(changed) && (threadIdx.x & 63) == 0) f.hdr[16 + r] = 1;
}

__global__ __launch_bounds__(TPB) void png_gather_kernel(File f) {
    if (f.hdr[0]) return;
    const uint32_t i = blockIdx.x * (uint32_t)TPB + threadIdx.x;
    if (i < f.N) f.bytes[i] = f.lit[min(f.src[i], i)];
}

__global__ __launch_bounds__(TPB) void png_adler_kernel(File f) {
    if (f.hdr[0]) return;
    __shared__ unsigned long long sa, sb;
    if (threadIdx.x == 0) sa = 0, sb = 0;
    __syncthreads();
    const uint32_t c0 = blockIdx.x * (uint32_t)IR_PNG_ADLER_CHUNK, len = min((uint32_t)IR_PNG_ADLER_CHUNK, f.N - c0);
    unsigned long long a = 0, b = 0;
    for (uint32_t j = threadIdx.x * 64u; j < min(len, threadIdx.x * 64u + 64u); ++j) {
        const uint32_t d = f.bytes[c0 + j];
        a += d, b += (unsigned long long)(len - j) * d;
    }
    atomicAdd(&sa, a), atomicAdd(&sb, b);
    __syncthreads();
    if (threadIdx.x == 0) f.asum[2 * blockIdx.x] = (uint32_t)(sa % 65521), f.asum[2 * blockIdx.x + 1] = (uint32_t)(sb % 65521);
}

__global__ void png_adler_join_kernel(File f, uint32_t chunks) {
    if (threadIdx.x || blockIdx.x || f.hdr[0]) return;
    unsigned long long a = 1, b = 0;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t len = min((uint32_t)IR_PNG_ADLER_CHUNK, f.N - c * (uint32_t)IR_PNG_ADLER_CHUNK);
        b = (b + len * a + f.asum[2 * c + 1]) % 65521;
        a = (a + f.asum[2 * c]) % 65521;
    }
    const uint32_t got = (uint32_t)((b << 16) | a);
    f.hdr[3] = got;
    if (got != f.adler) f.hdr[0] = E_ADLER;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {   // bytes: |x - y| is one v_sad_u32
    const unsigned pa = __usad(b, c, 0), pb = __usad(a, c, 0), pc = __usad(a + b, 2 * c, 0);
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}

constexpr int UL = IR_PNG_UNFILTER_LANES;
template <int BPP>
__global__ __launch_bounds__(UL) void png_unfilter_kernel(File f) {
    if (f.hdr[0]) return;
    constexpr int G = 4 * BPP, GW = BPP;   // a group: 4 pixels, G bytes, GW words
    __shared__ uint32_t slot[2][UL][GW];
    const int r = threadIdx.x, wk = (f.w + 3) / 4, P = max(wk, UL), nj = (f.h + UL - 1) / UL;
    const int steps = (nj - 1) * P + UL - 1 + wk, stride = f.rb + 1;
    int left[BPP], ul[BPP], ftype = 0;
    bool bad = false;
    for (int t = 0; t < steps; ++t) {
        const int tt = t - r, j = tt >= 0 ? tt / P : 0, g = tt >= 0 ? tt % P : 0, row = r + j * UL;
        if (tt >= 0 && row < f.h && g < wk) {
            const size_t at = (size_t)row * stride;
            if (g == 0) {
                ftype = f.bytes[at];
                if (ftype > 4) bad = true, ftype = 0;
                for (int c = 0; c < BPP; ++c) left[c] = ul[c] = 0;
            }
            uint32_t up[GW], cur[GW], res[GW];
            const size_t in = at + 1 + (size_t)g * G;   // any alignment: the aligned words around it (the section has room behind its end)
            const uint32_t* wp = reinterpret_cast<const uint32_t*>(f.bytes + (in & ~(size_t)3));
            const int sh = 8 * (int)(in & 3);
            uint32_t lo = wp[0];
            for (int k = 0; k < GW; ++k) {
                const uint32_t hi = wp[k + 1];
                cur[k] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh), lo = hi;
            }
            for (int k = 0; k < GW; ++k)
                up[k] = row == 0 ? 0u : r > 0 ? slot[(t - 1) & 1][r - 1][k] : reinterpret_cast<const uint32_t*>(f.pix + (size_t)(row - 1) * f.ppitch)[g * GW + k];
            for (int k = 0; k < GW; ++k) res[k] = 0;
            // one instantiation per filter type, so that a row pays for its own predictor alone; cc is the byte above of one pixel earlier
            auto run = [&](auto type) {
                constexpr int FT = decltype(type)::value;
                for (int b = 0; b < G; ++b) {
                    const int c = b % BPP, a = left[c], cc = ul[c];
                    const int x = __builtin_amdgcn_ubfe(cur[b >> 2], 8 * (b & 3), 8), bb = __builtin_amdgcn_ubfe(up[b >> 2], 8 * (b & 3), 8);
                    const int add = FT == 0 ? 0 : FT == 1 ? a : FT == 2 ? bb : FT == 3 ? (a + bb) >> 1 : paeth(a, bb, cc);
                    const int val = (x + add) & 255;
                    left[c] = val, ul[c] = bb;
                    res[b >> 2] |= (uint32_t)val << (8 * (b & 3));
                }
            };
            switch (ftype) {
                case 0: run(std::integral_constant<int, 0>{}); break;
                case 1: run(std::integral_constant<int, 1>{}); break;
                case 2: run(std::integral_constant<int, 2>{}); break;
                case 3: run(std::integral_constant<int, 3>{}); break;
                default: run(std::integral_constant<int, 4>{}); break;
            }
            uint32_t* po = reinterpret_cast<uint32_t*>(f.pix + (size_t)row * f.ppitch) + g * GW;
            for (int k = 0; k < GW; ++k) slot[t & 1][r][k] = res[k], po[k] = res[k];
        }
        __syncthreads();
    }
    if (bad) atomicCAS(&f.hdr[0], 0u, (uint32_t)E_FILTER);
}

__global__ __launch_bounds__(TPB) void png_rgb_kernel(File f, uint8_t* __restrict__ out, long pitch, uint32_t* __restrict__ info) {
    const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
    if (i == 0) *info = f.hdr[0];
    if (f.hdr[0] || i >= (size_t)f.h * f.w) return;
    const int y = (int)(i / f.w), x = (int)(i % f.w);
    const uint8_t* p = f.pix + (size_t)y * f.ppitch + (size_t)x * f.bpp;
    uint8_t* o = out + (size_t)y * pitch + 3 * (size_t)x;
    const bool grey = f.bpp < 3;
    o[0] = p[0], o[1] = grey ? p[0] : p[1], o[2] = grey ? p[0] : p[2];
}

int bpp_of(int color_type) { return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0; }
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int ir_png_decode_check(const ir_png_file* f, const char** why) {
    auto bad = [why](const char* w) { *why = w; return -1; };
    if (!f->stream || !f->out) return bad("null pointer in the record");
    if (f->h < 1 || f->w < 1 || f->h > 65535 || f->w > 65535 || (long)f->h * (1 + 4L * f->w) >= (1L << 31)) return bad("sides outside 1 .. 65535, or h (1 + 4 w) not below 2^31");
    if (!bpp_of(f->color_type)) return bad("colour type other than 0, 2, 4, 6");
    if (f->pitch < 3L * f->w) return bad("pitch below 3 w");
    if (f->stream_bytes < 8 || (f->stream_bytes & 3) || f->stream_bytes > (1u << 28)) return bad("stream_bytes no multiple of 4 in 8 .. 2^28");
    if (reinterpret_cast<uintptr_t>(f->stream) & 3) return bad("misaligned stream");
    return 0;
}

bool ir_png_decode_layout(int h, int w, uint32_t stream_bytes, int span_bits, IrPngLayout* L) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || (long)h * (1 + 4L * w) >= (1L << 31) || span_bits < 256 || span_bits > (1 << 20) || span_bits % 32 ||
        stream_bytes < 8 || (stream_bytes & 3) || stream_bytes > (1u << 28))
        return false;
    L->spans = ((size_t)stream_bytes * 8 + span_bits - 1) / span_bits, L->entries = L->spans + 1;
    L->cap = (size_t)h * (1 + 4 * (size_t)w), L->chunks = (L->cap + IR_PNG_ADLER_CHUNK - 1) / IR_PNG_ADLER_CHUNK;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += up256(bytes); return o; };
    L->hdr = take(256), L->cand = take(4 * L->spans);
    L->e_end = take(4 * L->entries), L->e_next = take(4 * L->entries), L->e_len = take(4 * L->entries), L->e_status = take(4 * L->entries);
    L->e_off = take(4 * L->entries), L->chain = take(4 * L->entries);
    L->adler = take(8 * L->chunks), L->src = take(4 * L->cap), L->lit = take(L->cap), L->bytes = take(L->cap + 32);
    L->pix = take((size_t)h * (4 * (size_t)w + 32));
    L->total = at;
    return true;
}

size_t ir_png_decode_workspace(int h, int w, uint32_t stream_bytes, int span_bits) {
    IrPngLayout L;
    return ir_png_decode_layout(h, w, stream_bytes, span_bits, &L) ? L.total : 0;
}

int ir_launch_png_decode(const ir_png_file* r, int span_bits, uint32_t* info, void* ws, const IrPngLayout& L, hipStream_t s) {
    const char* why;
    if (ir_png_decode_check(r, &why)) return -1;
    uint8_t* b = static_cast<uint8_t*>(ws);
    File f;
    f.words = reinterpret_cast<const uint32_t*>(r->stream);
    f.nwords = r->stream_bytes / 4, f.nbits = r->stream_bytes * 8, f.span = (uint32_t)span_bits;
    f.spans = (f.nbits + f.span - 1) / f.span, f.entries = f.spans + 1;
    f.h = r->h, f.w = r->w, f.bpp = bpp_of(r->color_type), f.rb = f.w * f.bpp, f.ppitch = ((f.rb + 15) & ~15) + 16;
    f.N = (uint32_t)r->h * (uint32_t)(1 + f.rb), f.adler = r->adler;
    if (f.spans > L.spans || f.N > L.cap || (size_t)f.h * f.ppitch > (size_t)f.h * (4 * (size_t)f.w + 32)) return -1;
    auto u32 = [b](size_t o) { return reinterpret_cast<uint32_t*>(b + o); };
    f.hdr = u32(L.hdr), f.cand = u32(L.cand), f.e_end = u32(L.e_end), f.e_next = u32(L.e_next), f.e_len = u32(L.e_len), f.e_status = u32(L.e_status);
    f.e_off = u32(L.e_off), f.chain = u32(L.chain), f.asum = u32(L.adler), f.src = u32(L.src);
    f.lit = b + L.lit, f.bytes = b + L.bytes, f.pix = b + L.pix;
    if (hipMemsetAsync(f.hdr, 0, 256, s) != hipSuccess || hipMemsetAsync(f.cand, 0xff, 4 * (size_t)f.spans, s) != hipSuccess) return -1;
    auto grid = [](size_t n, size_t per) { return dim3((unsigned)((n + per - 1) / per)); };
    hipLaunchKernelGGL(png_find_kernel, grid(f.nbits, FIND_RUN), dim3(64), 0, s, f);
    hipLaunchKernelGGL(png_walk_kernel<false>, dim3(f.entries), dim3(64), 0, s, f);
    hipLaunchKernelGGL(png_chain_kernel, dim3(1), dim3(64), 0, s, f);
    hipLaunchKernelGGL(png_walk_kernel<true>, dim3(f.entries), dim3(64), 0, s, f);
    int rounds = 0;
    while ((1ull << rounds) < f.N) ++rounds;
    for (int k = 0; k < rounds; ++k) hipLaunchKernelGGL(png_round_kernel, grid(f.N, TPB), dim3(TPB), 0, s, f, k);
    hipLaunchKernelGGL(png_gather_kernel, grid(f.N, TPB), dim3(TPB), 0, s, f);
    const uint32_t chunks = (f.N + IR_PNG_ADLER_CHUNK - 1) / IR_PNG_ADLER_CHUNK;
    hipLaunchKernelGGL(png_adler_kernel, dim3(chunks), dim3(TPB), 0, s, f);
    hipLaunchKernelGGL(png_adler_join_kernel, dim3(1), dim3(64), 0, s, f, chunks);
    switch (f.bpp) {
        case 1: hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3(1), dim3(UL), 0, s, f); break;
        case 2: hipLaunchKernelGGL(png_unfilter_kernel<2>, dim3(1), dim3(UL), 0, s, f); break;
        case 3: hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3(1), dim3(UL), 0, s, f); break;
        default: hipLaunchKernelGGL(png_unfilter_kernel<4>, dim3(1), dim3(UL), 0, s, f); break;
    }
    hipLaunchKernelGGL(png_rgb_kernel, grid((size_t)f.h * f.w, TPB), dim3(TPB), 0, s, f, r->out, r->pitch, info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
