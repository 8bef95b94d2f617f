// Lossless PNG scanline encoding of uint8 HWC RGB device images (ir_png_encode): Paeth filter + one dynamic-Huffman deflate block of
// literals per chunk of IR_PNG_ROWS rows, no matches. Per image the output is a complete zlib stream (header, blocks, Adler-32); the
// host adds the PNG chunk framing and its CRC (instarevive_amd/png.py). Format per chunk:
//   block header, 1106 bits: BFINAL, BTYPE = 10, HLIT = 257, HDIST = 1, HCLEN = 19, the code-length alphabet with symbols 0..15 at
//     length 4 and 16..18 at length 0 (a complete code: every literal length goes out as 4 plain bits), 257 literal lengths, one
//     distance length 0 (RFC 1951 allows it when no distance is used)
//   the literals of the filtered rows, the end-of-block symbol
//   every chunk but the last: an empty stored block (000, pad to the byte, 00 00 FF FF) so that the next chunk starts on a byte
// Four launches in stream order, because each consumes what other workgroups of the previous one produced (the per-XCD L2s are not
// coherent inside a launch): histograms + Adler partials, code construction, encode into a 16-byte aligned slot per chunk, compaction.
// The residuals are recomputed from the image in the first and third launch, never stored.
// The run mode (ir_png_encode_runs, the file's second half) adds matches at distance 1 for runs of equal filtered bytes and a compacted block
// header, and per chunk writes whichever of the two blocks is shorter; it shares this half's filter, literal-only coder and compaction, and
// this half's kernels and the bytes ir_png_encode writes are what they were without it.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int ROWS = IR_PNG_ROWS;
constexpr int HDR_BITS = IR_PNG_HEADER_BITS;
constexpr int NSYM = 257, EOB = 256, MAXLEN = 15;
constexpr int RUN = 16;                     // residual bytes per lane and tile
constexpr int TPB = 256;                    // threads of the histogram / encode / compact workgroups
constexpr int TILE = TPB * RUN;             // bytes per tile
constexpr int BUF_WORDS = 40 + TILE * MAXLEN / 32 + 8;   // the header (first tile) or the carried 16-byte unit + a tile's bits at 15 per byte + the chunk's tail
constexpr uint32_t ADLER = 65521;

struct Geo {
    const uint8_t* img;   // image 0, row 0
    long pitch, img_stride;
    int vh, vw, rowlen, chunks;
};

IR_DEVINL int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// OR nb <= 32 bits of v into an LDS bit array at bit pos (LSB first, deflate's order)
IR_DEVINL void put_bits(uint32_t* buf, uint32_t pos, unsigned long long v, int nb) {
    if (!nb) return;
    const uint32_t w = pos >> 5, sh = pos & 31;
    const unsigned long long x = v << sh;
    atomicOr(&buf[w], (uint32_t)x);
    if (sh + nb > 32) atomicOr(&buf[w + 1], (uint32_t)(x >> 32));
}

// RUN bytes of the filtered stream of one image from (row, col) on, col counting the filter-type byte as 0; the run may cross rows.
// Bytes from `count` on are not read and left 0.
IR_DEVINL void filtered_run(const uint8_t* img, long pitch, int rowlen, int row, int col, int count, uint8_t (&d)[RUN]) {
    const uint8_t* cur = img + (long)row * pitch;
    if (count == RUN && col >= 1 && col + RUN <= rowlen) {   // inside one row's pixel bytes: every byte loaded once
        const int x0 = col - 1;
        int c[RUN + 3], u[RUN + 3];
#pragma unroll
        for (int j = 0; j < RUN + 3; ++j) {
            const int x = x0 + j - 3;
            c[j] = x >= 0 ? cur[x] : 0;
            u[j] = (x >= 0 && row > 0) ? cur[x - pitch] : 0;
        }
#pragma unroll
        for (int j = 0; j < RUN; ++j) d[j] = (uint8_t)(c[j + 3] - paeth(c[j], u[j + 3], u[j]));
        return;
    }
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        d[j] = 0;
        if (j < count) {
            if (col == 0) d[j] = 4;
            else {
                const int x = col - 1;
                const int a = x >= 3 ? cur[x - 3] : 0, b = row > 0 ? cur[x - pitch] : 0, cc = (x >= 3 && row > 0) ? cur[x - pitch - 3] : 0;
                d[j] = (uint8_t)(cur[x] - paeth(a, b, cc));
            }
            if (++col == rowlen) { col = 0; ++row; cur += pitch; }
        }
    }
}

// ---------------------------------------------------------------- 1. histograms + Adler-32 partials, one workgroup per chunk
// hist[chunk][260]: 257 counters (the end-of-block symbol counted once), then s1 = sum of bytes, s2 = sum of (len - k) * byte[k], both mod 65521
__global__ __launch_bounds__(TPB) void png_hist_kernel(Geo g, uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[TPB / 64][NSYM + 3];
    __shared__ unsigned long long red[2][TPB / 64];
    const int chunk = blockIdx.x, image = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const uint8_t* img = g.img + image * g.img_stride;
    const int row0 = chunk * ROWS, rows = min(ROWS, g.vh - row0);
    const int len = rows * g.rowlen;
    for (int i = tid; i < (TPB / 64) * (NSYM + 3); i += TPB) (&cnt[0][0])[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int k0 = tid * RUN; k0 < len; k0 += TILE) {
        uint8_t d[RUN];
        const int r = k0 / g.rowlen;
        filtered_run(img, g.pitch, g.rowlen, row0 + r, k0 - r * g.rowlen, min(RUN, len - k0), d);
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (k0 + j < len) {
                atomicAdd(&cnt[wave][d[j]], 1u);
                s1 += d[j];
                s2 += (unsigned long long)(len - k0 - j) * d[j];
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
    }
    if ((tid & 63) == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    uint32_t* out = hist + ((long)image * g.chunks + chunk) * 260;
    for (int s = tid; s < NSYM; s += TPB) {
        uint32_t v = s == EOB ? 1u : 0u;
        for (int w = 0; w < TPB / 64; ++w) v += cnt[w][s];
        out[s] = v;
    }
    if (tid < 2) {
        unsigned long long t = 0;
        for (int w = 0; w < TPB / 64; ++w) t += red[tid][w];
        out[NSYM + tid] = (uint32_t)(t % ADLER);
    }
}

// ---------------------------------------------------------------- 2. code construction, one wave per chunk
// codes[chunk][260]: per symbol (bit-reversed canonical code) | length << 16; header[chunk][40]: the 1106 header bits; chunk_bytes[chunk].
// Huffman lengths of the histogram; while the longest exceeds 15 the histogram is halved with a floor of 1 and the tree rebuilt
// (deterministic: ties are ordered by symbol, and a leaf goes before an internal node of equal weight). The code never costs more than
// the fixed code "8 bits for 0..254, 9 for 255 and end-of-block" (complete: 255/256 + 2/512 = 1): where a halved histogram's code would,
// that fixed code is taken, which is what makes ir_png_bound's 9 bits per byte hold for any pixels.
// The construction itself, shared with the run mode's code kernel: one wave, N symbols. freq: the histogram, written by the caller's lanes
// (no barrier needed in between) and halved here; len: the result.
template <int N>
struct Huffman {
    uint32_t freq[N], sfreq[N], nfreq[N];
    uint16_t ssym[N], pleaf[N], pnode[N];
    uint8_t len[N + 3];
    int n, deepest;
};
template <int N>
IR_DEVINL void limited_huffman_lengths(Huffman<N>& h) {
    uint32_t(&freq)[N] = h.freq, (&sfreq)[N] = h.sfreq, (&nfreq)[N] = h.nfreq;
    uint16_t(&ssym)[N] = h.ssym, (&pleaf)[N] = h.pleaf, (&pnode)[N] = h.pnode;
    uint8_t(&len)[N + 3] = h.len;
    const int lane = threadIdx.x;
    if (lane == 0) h.n = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int s = lane; s < N; s += 64) mine += freq[s] > 0;
        atomicAdd(&h.n, mine);
    }
    __syncthreads();
    const int n = h.n;   // >= 2: the chunk's first byte and the end-of-block symbol always occur
    for (;;) {
        // rank sort of the used symbols by (count, symbol)
        for (int s = lane; s < N; s += 64) {
            const uint32_t f = freq[s];
            len[s] = 0;
            if (!f) continue;
            int rank = 0;
            for (int t = 0; t < N; ++t) {
                const uint32_t ft = freq[t];
                rank += ft && (ft < f || (ft == f && t < s));
            }
            ssym[rank] = (uint16_t)s;
            sfreq[rank] = f;
        }
        if (lane == 0) h.deepest = 0;
        __syncthreads();
        if (lane == 0) {   // two-queue merge: leaves in sorted order, internal nodes in creation order (their weights never decrease)
            int i = 0, j = 0;
            for (int k = 0; k < n - 1; ++k) {
                uint32_t w = 0;
                for (int pick = 0; pick < 2; ++pick) {
                    if (i < n && (j >= k || sfreq[i] <= nfreq[j])) { w += sfreq[i]; pleaf[i++] = (uint16_t)k; }
                    else { w += nfreq[j]; pnode[j++] = (uint16_t)k; }
                }
                nfreq[k] = w;
            }
        }
        __syncthreads();
        int deepest = 0;
        for (int r = lane; r < n; r += 64) {   // depth of leaf r = hops to the root (node n - 2)
            int d = 1;
            for (int p = pleaf[r]; p != n - 2; p = pnode[p]) ++d;
            len[ssym[r]] = (uint8_t)min(d, 255);
            deepest = max(deepest, d);
        }
        atomicMax(&h.deepest, deepest);
        __syncthreads();
        if (h.deepest <= MAXLEN) break;
        for (int s = lane; s < N; s += 64)
            if (freq[s]) freq[s] = max(1u, freq[s] >> 1);
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void png_codes_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ codes, uint32_t* __restrict__ header,
                                                       uint32_t* __restrict__ chunk_bytes, int chunks) {
    __shared__ Huffman<NSYM> huff;
    __shared__ uint32_t orig[NSYM];
    __shared__ uint32_t hdr[40], next_code[MAXLEN + 2], blc[MAXLEN + 2];
    __shared__ unsigned long long sh_bits[2];
    uint8_t(&len)[NSYM + 3] = huff.len;
    const int lane = threadIdx.x;
    const long slot = (long)blockIdx.y * chunks + blockIdx.x;
    const bool last = blockIdx.x == chunks - 1;
    hist += slot * 260;
    for (int s = lane; s < NSYM; s += 64) orig[s] = huff.freq[s] = hist[s];
    limited_huffman_lengths(huff);
    // cost on the chunk's real histogram against the fixed code
    unsigned long long bits = 0, fixed = 0;
    for (int s = lane; s < NSYM; s += 64) {
        bits += (unsigned long long)orig[s] * len[s];
        fixed += (unsigned long long)orig[s] * (s < 255 ? 8 : 9);
    }
    for (int o = 32; o > 0; o >>= 1) {
        bits += __shfl_down(bits, o, 64);
        fixed += __shfl_down(fixed, o, 64);
    }
    if (lane == 0) { sh_bits[0] = bits; sh_bits[1] = fixed; }
    if (lane < MAXLEN + 2) blc[lane] = 0;
    if (lane < 40) hdr[lane] = 0;
    __syncthreads();
    const bool use_fixed = sh_bits[0] > sh_bits[1];
    if (use_fixed)
        for (int s = lane; s < NSYM; s += 64) len[s] = s < 255 ? 8 : 9;
    __syncthreads();
    for (int s = lane; s < NSYM; s += 64)
        if (len[s]) atomicAdd(&blc[len[s]], 1u);
    __syncthreads();
    if (lane == 0) {
        uint32_t code = 0;
        blc[0] = 0;
        for (int l = 1; l <= MAXLEN; ++l) {
            code = (code + blc[l - 1]) << 1;
            next_code[l] = code;
        }
        // BFINAL | BTYPE = 2 | HLIT = 0 (257) | HDIST = 0 (1) | HCLEN = 15 (19), LSB first: 17 bits, then 19 x 3 bits of the code-length alphabet in
        // the order 16 17 18 0 8 7 ...: the first three are 0, the other sixteen 4
        put_bits(hdr, 0, (last ? 1u : 0u) | (2u << 1) | (15u << 13), 17);
        for (int i = 3; i < 19; ++i) put_bits(hdr, 17 + 3 * i, 4, 3);
    }
    __syncthreads();
    for (int s = lane; s < NSYM; s += 64) {
        const int l = len[s];
        uint32_t cw = 0;
        if (l) {
            int before = 0;
            for (int t = 0; t < s; ++t) before += len[t] == l;
            cw = __brev(next_code[l] + before) >> (32 - l);
        }
        codes[slot * 260 + s] = cw | ((uint32_t)l << 16);
        // bits 17 + 57 = 74 .. : the literal lengths, each the 4-bit code of its value (symbol v of the code-length alphabet has code v), MSB first
        put_bits(hdr, 74 + 4 * s, __brev((uint32_t)l) >> 28, 4);
    }
    __syncthreads();   // (the distance length, 4 zero bits at 74 + 4 * 257 = 1102, needs no write)
    if (lane < 40) header[slot * 40 + lane] = hdr[lane];
    if (lane == 0) {
        const unsigned long long body = HDR_BITS + (use_fixed ? sh_bits[1] : sh_bits[0]);
        chunk_bytes[slot] = (uint32_t)(last ? (body + 7) / 8 : (body + 3 + 7) / 8 + 4);
    }
}

// ---------------------------------------------------------------- 3. encode, one workgroup per chunk
// Tiles of TPB x RUN residual bytes: each lane sums the bit counts of its run, the block prefix sum places it, the lanes OR their bits into
// an LDS window that starts on a 16-byte boundary of the chunk's stream, and the window's finished 16-byte units go out as dwordx4 stores.
IR_DEVINL void encode_literal_chunk(const Geo& g, const uint32_t* __restrict__ codes, const uint32_t* __restrict__ header, uint8_t* __restrict__ slots,
                                    long slot_cap) {
    __shared__ uint32_t code[NSYM + 3];
    __shared__ __attribute__((aligned(16))) uint32_t buf[BUF_WORDS];
    __shared__ uint32_t wsum[TPB / 64];
    const int chunk = blockIdx.x, image = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = (long)image * g.chunks + chunk;
    const uint8_t* img = g.img + image * g.img_stride;
    uint4* dst = reinterpret_cast<uint4*>(slots + slot * slot_cap);
    const int row0 = chunk * ROWS, rows = min(ROWS, g.vh - row0);
    const int len = rows * g.rowlen;
    const bool last = chunk == g.chunks - 1;
    for (int i = tid; i < NSYM; i += TPB) code[i] = codes[slot * 260 + i];
    for (int i = tid; i < BUF_WORDS; i += TPB) buf[i] = i < 40 ? header[slot * 40 + i] : 0u;   // words 35..39 of the header are 0
    __syncthreads();
    uint32_t P = HDR_BITS;     // bits of the chunk's stream so far
    uint32_t unit0 = 0;        // 16-byte units already stored; the window starts at bit unit0 * 128
    for (int t0 = 0; t0 <= len; t0 += TILE) {   // (<=: an exact multiple still runs the tail step below once)
        const int k0 = t0 + tid * RUN;
        const int count = max(0, min(RUN, len - k0));
        uint8_t d[RUN];
        uint32_t nbits = 0;
        if (count > 0) {
            const int r = k0 / g.rowlen;
            filtered_run(img, g.pitch, g.rowlen, row0 + r, k0 - r * g.rowlen, count, d);
#pragma unroll
            for (int j = 0; j < RUN; ++j)
                if (j < count) nbits += code[d[j]] >> 16;
        }
        uint32_t incl = nbits;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < TPB / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (count > 0) {
            uint32_t pos = P - unit0 * 128 + before + incl - nbits;
            unsigned long long acc = 0;
            int fill = 0;
#pragma unroll
            for (int j = 0; j < RUN; ++j)
                if (j < count) {
                    const uint32_t cw = code[d[j]];
                    acc |= (unsigned long long)(cw & 0xffff) << fill;
                    fill += cw >> 16;
                    if (fill >= 32) {
                        put_bits(buf, pos, acc & 0xffffffffull, 32);
                        pos += 32; acc >>= 32; fill -= 32;
                    }
                }
            put_bits(buf, pos, acc, fill);
        }
        P += total;
        const bool tail = t0 + TILE > len;   // the last tile: end-of-block and the chunk's closing bytes
        __syncthreads();
        if (tail && tid == 0) {
            const uint32_t e = code[EOB];
            put_bits(buf, P - unit0 * 128, e & 0xffff, e >> 16);
            P += e >> 16;
            if (!last) {
                P = ((P + 3 + 7) & ~7u) + 16;           // 000, pad to the byte, 00 00 ...
                put_bits(buf, P - unit0 * 128, 0xffff, 16);   // ... FF FF
                P += 16;
            } else {
                P = (P + 7) & ~7u;
            }
            wsum[0] = P;
        }
        if (tail) {
            __syncthreads();
            P = wsum[0];
        }
        const uint32_t units = tail ? (P + 127) / 128 - unit0 : P / 128 - unit0;   // the tail stores its partial unit too (zero padded, inside the slot)
        for (uint32_t u = tid; u < units; u += TPB) dst[unit0 + u] = reinterpret_cast<const uint4*>(buf)[u];
        if (tail) break;
        // carry the unfinished unit to the window's start and clear the rest
        uint32_t keep = 0;
        if (tid < 4) keep = buf[units * 4 + tid];
        __syncthreads();
        for (int i = tid; i < BUF_WORDS; i += TPB) buf[i] = 0;
        __syncthreads();
        if (tid < 4) buf[tid] = keep;
        unit0 += units;
        __syncthreads();
    }
}
__global__ __launch_bounds__(TPB) void png_encode_kernel(Geo g, const uint32_t* __restrict__ codes, const uint32_t* __restrict__ header,
                                                         uint8_t* __restrict__ slots, long slot_cap) {
    encode_literal_chunk(g, codes, header, slots, slot_cap);
}

// ---------------------------------------------------------------- 4. compact, one workgroup per chunk
// out[image]: 78 01 | the chunks back to back | Adler-32 (big endian); info[image] = the stream's byte count. Nothing behind it is written.
__global__ __launch_bounds__(TPB) void png_compact_kernel(const uint8_t* __restrict__ slots, long slot_cap, const uint32_t* __restrict__ chunk_bytes,
                                                          const uint32_t* __restrict__ hist, uint8_t* __restrict__ out, size_t out_stride,
                                                          uint32_t* __restrict__ info, int chunks, int rows_total, int rowlen) {
    __shared__ unsigned long long red[TPB / 64];
    const int chunk = blockIdx.x, image = blockIdx.y, tid = threadIdx.x;
    const long base = (long)image * chunks;
    unsigned long long off = 0;
    for (int c = tid; c < chunk; c += TPB) off += chunk_bytes[base + c];
    for (int o = 32; o > 0; o >>= 1) off += __shfl_down(off, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = off;
    __syncthreads();
    off = 0;
    for (int w = 0; w < TPB / 64; ++w) off += red[w];
    const uint32_t nbytes = chunk_bytes[base + chunk];
    uint8_t* img_out = out + (size_t)image * out_stride;
    uint8_t* dst = img_out + 2 + off;
    const uint8_t* src = slots + (base + chunk) * slot_cap;   // 16-byte aligned, readable up to slot_cap
    // head bytes up to the first 4-byte aligned destination address, whole dwords, tail bytes
    const uint32_t head = min(nbytes, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
    const uint32_t words = (nbytes - head) / 4, tail0 = head + words * 4;
    if (tid < head) dst[tid] = src[tid];
    if (tid >= 64 && tid - 64 < nbytes - tail0) dst[tail0 + tid - 64] = src[tail0 + tid - 64];
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    const uint32_t sh = (head & 3) * 8;   // source byte head + 4 i sits at byte (head & 3) of source word (head >> 2) + i
    for (uint32_t i = tid; i < words; i += TPB) {
        const uint32_t lo = sw[(head >> 2) + i];
        uint32_t v = lo;
        if (sh) v = (lo >> sh) | (sw[(head >> 2) + i + 1] << (32 - sh));
        dw[i] = v;
    }
    if (chunk == chunks - 1 && tid == 0) {
        uint32_t a = 1, b = 0;
        for (int c = 0; c < chunks; ++c) {   // (s1, s2, len) of the chunks in order
            const uint32_t len = (uint32_t)(min(IR_PNG_ROWS, rows_total - c * IR_PNG_ROWS)) * rowlen;
            const uint32_t s1 = hist[(base + c) * 260 + NSYM], s2 = hist[(base + c) * 260 + NSYM + 1];
            b = (uint32_t)((b + (unsigned long long)(len % ADLER) * a + s2) % ADLER);
            a = (a + s1) % ADLER;
        }
        img_out[0] = 0x78;
        img_out[1] = 0x01;
        uint8_t* tr = dst + nbytes;
        tr[0] = (uint8_t)(b >> 8); tr[1] = (uint8_t)b; tr[2] = (uint8_t)(a >> 8); tr[3] = (uint8_t)a;
        info[image] = (uint32_t)(2 + off + nbytes + 4);
    }
}

// ================================================================ the run mode (ir_png_encode_runs)
// Inside a chunk every maximal run of equal filtered bytes (filter-type bytes included, rows crossed, the chunk's boundary never) is one literal,
// then matches at distance 1: pieces of 258 bytes, and the remainder as one match if it has RMIN bytes, as literals otherwise. A byte at offset
// k >= 1 of its run therefore sits in the piece that starts m = (k - 1) % 258 bytes before it and has min(258, run end - piece start) bytes: it is
// the piece's head (m == 0) and emits the match, or emits nothing, or - piece shorter than RMIN - a literal. It needs its run's start, which is
// the last byte at or before it that differs from its predecessor, and its run's end no further than 258 bytes behind the piece's start. The
// first launch marks those bytes in a bit mask (one bit per byte, the chunk's end marked as well), kept in the LDS and in the workspace for the
// third launch; the start comes from a block-wide max scan of each lane's last mark, carried from tile to tile, the end from the marks ahead.
// A run-coded chunk is one dynamic-Huffman block of 286 literal / length codes and ONE distance code of one bit. Its code lengths go out under a
// fixed complete code of the code-length alphabet (18: 3 bits; 0, 3 .. 11, 17: 4 bits; 1, 2, 12 .. 15: 5 bits; 16 unused), stretches of zeros
// greedily as symbol 18 (11 .. 138) and 17 (3 .. 10). The second launch's own kernel compares the block's bits with the literal-only block's of
// png_codes_kernel and sets the chunk's choice: run-coded only where strictly cheaper, so no stream grows and ir_png_bound and the slots hold.
constexpr int RMIN = 6, RMAX = 258;
constexpr int RSYM = 286;                      // literal / length symbols
constexpr int RSTRIDE = IR_PNG_RUNS_SYMS;      // dwords per chunk of run_hist and run_codes; run_codes[RSYM] = the header's bits, [RSYM + 1] = 1: the chunk is run-coded
constexpr int RHDR_WORDS = IR_PNG_RUNS_HEADER_WORDS;
constexpr int FLAG_WORDS_MAX = (IR_PNG_RUNS_MAX_CHUNK + 32) / 32 + 12;
constexpr int RBITS = MAXLEN + 5 + 1;          // a match: length code, extra bits, the distance bit
constexpr int RBUF_WORDS = RHDR_WORDS + TILE * RBITS / 32 + 12;   // the header (first tile) or the carried unit + a tile's bits + the chunk's tail

IR_DEVINL int filtered_byte(const uint8_t* img, long pitch, int row, int col) {
    if (col == 0) return 4;
    const uint8_t* cur = img + (long)row * pitch;
    const int x = col - 1;
    const int a = x >= 3 ? cur[x - 3] : 0, b = row > 0 ? cur[x - pitch] : 0, cc = (x >= 3 && row > 0) ? cur[x - pitch - 3] : 0;
    return (uint8_t)(cur[x] - paeth(a, b, cc));
}

// match length 3 .. 258 -> symbol 257 .. 285, its extra bits' count and value (RFC 1951 section 3.2.5)
IR_DEVINL int length_symbol(int length, int& eb, int& extra) {
    const int l = length - 3;
    eb = 0; extra = 0;
    if (length == RMAX) return 285;
    if (l < 8) return 257 + l;
    eb = 29 - __clz(l);
    extra = l & ((1 << eb) - 1);
    return 261 + 4 * eb + ((l >> eb) & 3);
}
IR_DEVINL int length_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// first mark at or behind bit `from`; without one within 320 bits, a position beyond every piece that could reach it
IR_DEVINL int next_flag(const uint32_t* fl, int from) {
    int w = from >> 5;
    uint32_t v = fl[w] & (~0u << (from & 31));
    for (int i = 0; i < 10 && !v; ++i) v = fl[++w];
    return v ? (w << 5) + __ffs(v) - 1 : from + 512;
}

// The last mark before k0, the first byte of this lane's RUN bytes whose marks are fl16: max scan over the block, `carry` from the tiles before.
// Called by every thread of the block.
IR_DEVINL int run_start_before(uint32_t fl16, int k0, int& carry, int* wmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = fl16 ? k0 + 31 - __clz(fl16) : -1;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl = max(incl, v);
    }
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = -1;
    if (lane == 63) wmax[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < TPB / 64; ++w) {
        if (w < wave) before = max(before, wmax[w]);
        carry = max(carry, wmax[w]);
    }
    __syncthreads();   // wmax is written again by the next tile
    return max(before, excl);
}

// What each of the lane's bytes emits: emit(j, false, byte) for a literal, emit(j, true, length) for a match head, no call for a byte inside a match.
// s_in: run_start_before(); e_after: next_flag(k0 + RUN).
template <class F>
IR_DEVINL void classify(uint32_t fl16, int k0, int count, int s_in, int e_after, const uint8_t (&d)[RUN], F&& emit) {
    int cur_s = s_in;
#pragma unroll
    for (int j = 0; j < RUN; ++j)
        if (j < count) {
            const int i = k0 + j;
            if ((fl16 >> j) & 1) {
                cur_s = i;
                emit(j, false, (int)d[j]);
                continue;
            }
            const int m = (i - cur_s - 1) % RMAX, p = i - m;
            const uint32_t above = fl16 >> (j + 1);
            const int e = above ? i + __ffs(above) : e_after;
            const int piece = min(RMAX, e - p);
            if (piece < RMIN) emit(j, false, (int)d[j]);
            else if (m == 0) emit(j, true, piece);
        }
}

// ---------------------------------------------------------------- 1r. both histograms, the Adler-32 partials and the marks, one workgroup per chunk
// hist: png_hist_kernel's; run_hist[chunk][RSTRIDE]: the literal / length symbols of the chunk's parse, end-of-block counted once
__global__ __launch_bounds__(TPB) void png_runs_hist_kernel(Geo g, uint32_t* __restrict__ hist, uint32_t* __restrict__ run_hist, uint32_t* __restrict__ flags,
                                                            long flag_words) {
    __shared__ uint32_t fl[FLAG_WORDS_MAX];
    __shared__ uint32_t cnt[TPB / 64][NSYM + 3];
    __shared__ uint32_t rcnt[TPB / 64][RSTRIDE];
    __shared__ unsigned long long red[2][TPB / 64];
    __shared__ int wmax[TPB / 64];
    const int chunk = blockIdx.x, image = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const long slot = (long)image * g.chunks + chunk;
    const uint8_t* img = g.img + image * g.img_stride;
    const int row0 = chunk * ROWS, rows = min(ROWS, g.vh - row0);
    const int len = rows * g.rowlen;
    const int nwords = (len + 1 + 31) / 32 + 12;   // ir_png_runs_flag_words(len) <= flag_words
    for (int i = tid; i < (TPB / 64) * (NSYM + 3); i += TPB) (&cnt[0][0])[i] = 0;
    for (int i = tid; i < (TPB / 64) * RSTRIDE; i += TPB) (&rcnt[0][0])[i] = 0;
    for (int i = tid; i < nwords; i += TPB) fl[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int k0 = tid * RUN; k0 < len; k0 += TILE) {
        uint8_t d[RUN];
        const int r = k0 / g.rowlen;
        filtered_run(img, g.pitch, g.rowlen, row0 + r, k0 - r * g.rowlen, min(RUN, len - k0), d);
        int prev = -1;   // the chunk's first byte starts a run
        if (k0) {
            const int rp = (k0 - 1) / g.rowlen;
            prev = filtered_byte(img, g.pitch, row0 + rp, k0 - 1 - rp * g.rowlen);
        }
        uint32_t f = 0;
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (k0 + j < len) {
                atomicAdd(&cnt[wave][d[j]], 1u);
                s1 += d[j];
                s2 += (unsigned long long)(len - k0 - j) * d[j];
                f |= (uint32_t)(d[j] != prev) << j;
                prev = d[j];
            }
        reinterpret_cast<uint16_t*>(fl)[k0 >> 4] = (uint16_t)f;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
    }
    if ((tid & 63) == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (tid == 0) fl[len >> 5] |= 1u << (len & 31);   // the chunk's end closes the last run
    __syncthreads();
    for (int i = tid; i < nwords; i += TPB) flags[slot * flag_words + i] = fl[i];
    int carry = -1;
    for (int t0 = 0; t0 < len; t0 += TILE) {
        const int k0 = t0 + tid * RUN;
        const int count = max(0, min(RUN, len - k0));
        const uint32_t fl16 = count > 0 ? reinterpret_cast<const uint16_t*>(fl)[k0 >> 4] : 0u;
        const int s_in = run_start_before(fl16, k0, carry, wmax);
        if (count > 0) {
            uint8_t d[RUN];
            const int r = k0 / g.rowlen;
            filtered_run(img, g.pitch, g.rowlen, row0 + r, k0 - r * g.rowlen, count, d);
            classify(fl16, k0, count, s_in, next_flag(fl, k0 + RUN), d, [&](int, bool match, int v) {
                int eb, extra;
                atomicAdd(&rcnt[wave][match ? length_symbol(v, eb, extra) : v], 1u);
            });
        }
    }
    __syncthreads();
    uint32_t* out = hist + slot * 260;
    for (int s = tid; s < NSYM; s += TPB) {
        uint32_t v = s == EOB ? 1u : 0u;
        for (int w = 0; w < TPB / 64; ++w) v += cnt[w][s];
        out[s] = v;
    }
    if (tid < 2) {
        unsigned long long t = 0;
        for (int w = 0; w < TPB / 64; ++w) t += red[tid][w];
        out[NSYM + tid] = (uint32_t)(t % ADLER);
    }
    for (int s = tid; s < RSYM; s += TPB) {
        uint32_t v = s == EOB ? 1u : 0u;
        for (int w = 0; w < TPB / 64; ++w) v += rcnt[w][s];
        run_hist[slot * RSTRIDE + s] = v;
    }
}

// ---------------------------------------------------------------- 2r. the run-coded block's code, header and cost, and the chunk's choice; one wave per chunk
// Behind png_codes_kernel, whose codes give the literal-only block's bits. run_codes[chunk][RSTRIDE]: per symbol (bit-reversed canonical code) |
// length << 16, then the header's bit count and the choice; run_header[chunk][RHDR_WORDS]; chunk_bytes[chunk] is overwritten where the chunk is run-coded.
// The lengths are png_codes_kernel's construction on 286 symbols (limited_huffman_lengths), without the fixed code: a code that costs too much
// loses the chunk anyway.
IR_DEVINL uint32_t cl_code(int v, int& nb) {   // the code-length alphabet's fixed code, bit-reversed
    int c;
    if (v == 18) { c = 0; nb = 3; }
    else if (v == 0) { c = 2; nb = 4; }
    else if (v == 17) { c = 12; nb = 4; }
    else if (v >= 3 && v <= 11) { c = v; nb = 4; }
    else if (v <= 2) { c = 25 + v; nb = 5; }
    else { c = 16 + v; nb = 5; }   // 12 .. 15 -> 28 .. 31
    return __brev((uint32_t)c) >> (32 - nb);
}
__global__ __launch_bounds__(64) void png_runs_codes_kernel(const uint32_t* __restrict__ run_hist, const uint32_t* __restrict__ hist,
                                                            const uint32_t* __restrict__ codes, uint32_t* __restrict__ run_codes,
                                                            uint32_t* __restrict__ run_header, uint32_t* __restrict__ chunk_bytes, int chunks) {
    __shared__ Huffman<RSYM> huff;
    __shared__ uint32_t orig[RSYM];
    __shared__ uint32_t hdr[RHDR_WORDS], next_code[MAXLEN + 2], blc[MAXLEN + 2];
    __shared__ unsigned long long sh_bits[2];
    uint8_t(&len)[RSYM + 3] = huff.len;
    const int lane = threadIdx.x;
    const long slot = (long)blockIdx.y * chunks + blockIdx.x;
    const bool last = blockIdx.x == chunks - 1;
    run_hist += slot * RSTRIDE;
    for (int s = lane; s < RSYM; s += 64) orig[s] = huff.freq[s] = run_hist[s];
    limited_huffman_lengths(huff);
    // the symbols' bits (a length symbol: its code, its extra bits, the distance bit) and the literal-only block's
    unsigned long long bits = 0, lit = 0;
    for (int s = lane; s < RSYM; s += 64) {
        bits += (unsigned long long)orig[s] * (len[s] + (s > EOB ? length_extra_bits(s) + 1 : 0));
        if (s < NSYM) lit += (unsigned long long)hist[slot * 260 + s] * (codes[slot * 260 + s] >> 16);
    }
    for (int o = 32; o > 0; o >>= 1) {
        bits += __shfl_down(bits, o, 64);
        lit += __shfl_down(lit, o, 64);
    }
    if (lane == 0) { sh_bits[0] = bits; sh_bits[1] = lit + HDR_BITS; }
    if (lane < MAXLEN + 2) blc[lane] = 0;
    if (lane < RHDR_WORDS) hdr[lane] = 0;
    __syncthreads();
    for (int s = lane; s < RSYM; s += 64)
        if (len[s]) atomicAdd(&blc[len[s]], 1u);
    __syncthreads();
    if (lane == 0) {
        uint32_t code = 0;
        blc[0] = 0;
        for (int l = 1; l <= MAXLEN; ++l) {
            code = (code + blc[l - 1]) << 1;
            next_code[l] = code;
        }
        // BFINAL | BTYPE = 2 | HLIT = 29 (286) | HDIST = 0 (1) | HCLEN = 15 (19), then the code-length alphabet's lengths in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        put_bits(hdr, 0, (last ? 1u : 0u) | (2u << 1) | (29u << 3) | (15u << 13), 17);
        const uint8_t cl[19] = {0, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 5, 5, 5, 5, 5};
        for (int i = 0; i < 19; ++i) put_bits(hdr, 17 + 3 * i, cl[i], 3);
        // the 286 lengths and the distance code's 1
        uint32_t pos = 74;
        int nb;
        len[RSYM] = 1;
        for (int i = 0; i <= RSYM;) {
            const int v = len[i];
            if (v) {
                const uint32_t c = cl_code(v, nb);
                put_bits(hdr, pos, c, nb);
                pos += nb;
                ++i;
                continue;
            }
            int z = 0;
            while (i <= RSYM && !len[i]) { ++i; ++z; }
            while (z >= 11) {
                const int t = min(z, 138);
                const uint32_t c = cl_code(18, nb);
                put_bits(hdr, pos, c | ((uint32_t)(t - 11) << nb), nb + 7);
                pos += nb + 7;
                z -= t;
            }
            if (z >= 3) {
                const uint32_t c = cl_code(17, nb);
                put_bits(hdr, pos, c | ((uint32_t)(z - 3) << nb), nb + 3);
                pos += nb + 3;
                z = 0;
            }
            for (; z > 0; --z) {
                const uint32_t c = cl_code(0, nb);
                put_bits(hdr, pos, c, nb);
                pos += nb;
            }
        }
        const unsigned long long body = pos + sh_bits[0];
        const bool runs = body < sh_bits[1];
        run_codes[slot * RSTRIDE + RSYM] = pos;
        run_codes[slot * RSTRIDE + RSYM + 1] = runs ? 1u : 0u;
        if (runs) chunk_bytes[slot] = (uint32_t)(last ? (body + 7) / 8 : (body + 3 + 7) / 8 + 4);
    }
    __syncthreads();
    for (int s = lane; s < RSYM; s += 64) {
        const int l = len[s];
        uint32_t cw = 0;
        if (l) {
            int before = 0;
            for (int t = 0; t < s; ++t) before += len[t] == l;
            cw = __brev(next_code[l] + before) >> (32 - l);
        }
        run_codes[slot * RSTRIDE + s] = cw | ((uint32_t)l << 16);
    }
    if (lane < RHDR_WORDS) run_header[slot * RHDR_WORDS + lane] = hdr[lane];
}

// ---------------------------------------------------------------- 3r. encode, one workgroup per chunk: the block the chunk chose
// A run-coded chunk goes as png_encode_kernel's tiles do, with up to RBITS bits or none per byte: each lane packs what its bytes emit, the block
// prefix sum places it, the window's finished 16-byte units go out.
__global__ __launch_bounds__(TPB) void png_runs_encode_kernel(Geo g, const uint32_t* __restrict__ codes, const uint32_t* __restrict__ header,
                                                              uint8_t* __restrict__ slots, long slot_cap, const uint32_t* __restrict__ run_codes,
                                                              const uint32_t* __restrict__ run_header, const uint32_t* __restrict__ flags, long flag_words) {
    __shared__ uint32_t fl[FLAG_WORDS_MAX];
    __shared__ uint32_t code[RSTRIDE];
    __shared__ __attribute__((aligned(16))) uint32_t buf[RBUF_WORDS];
    __shared__ uint32_t wsum[TPB / 64];
    __shared__ int wmax[TPB / 64];
    const int chunk = blockIdx.x, image = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = (long)image * g.chunks + chunk;
    if (!run_codes[slot * RSTRIDE + RSYM + 1]) {   // the whole workgroup
        encode_literal_chunk(g, codes, header, slots, slot_cap);
        return;
    }
    const uint8_t* img = g.img + image * g.img_stride;
    uint4* dst = reinterpret_cast<uint4*>(slots + slot * slot_cap);
    const int row0 = chunk * ROWS, rows = min(ROWS, g.vh - row0);
    const int len = rows * g.rowlen;
    const int nwords = (len + 1 + 31) / 32 + 12;
    const bool last = chunk == g.chunks - 1;
    for (int i = tid; i < RSTRIDE; i += TPB) code[i] = run_codes[slot * RSTRIDE + i];
    for (int i = tid; i < RBUF_WORDS; i += TPB) buf[i] = i < RHDR_WORDS ? run_header[slot * RHDR_WORDS + i] : 0u;
    for (int i = tid; i < nwords; i += TPB) fl[i] = flags[slot * flag_words + i];
    __syncthreads();
    uint32_t P = code[RSYM];   // bits of the chunk's stream so far: the header
    uint32_t unit0 = 0;
    int carry = -1;
    for (int t0 = 0; t0 <= len; t0 += TILE) {
        const int k0 = t0 + tid * RUN;
        const int count = max(0, min(RUN, len - k0));
        const uint32_t fl16 = count > 0 ? reinterpret_cast<const uint16_t*>(fl)[k0 >> 4] : 0u;
        const int s_in = run_start_before(fl16, k0, carry, wmax);
        uint32_t tok[RUN];   // bits | count << 24 of what each byte emits
        uint32_t nbits = 0;
#pragma unroll
        for (int j = 0; j < RUN; ++j) tok[j] = 0;
        if (count > 0) {
            uint8_t d[RUN];
            const int r = k0 / g.rowlen;
            filtered_run(img, g.pitch, g.rowlen, row0 + r, k0 - r * g.rowlen, count, d);
            classify(fl16, k0, count, s_in, next_flag(fl, k0 + RUN), d, [&](int j, bool match, int v) {
                int eb = 0, extra = 0;
                const uint32_t cw = code[match ? length_symbol(v, eb, extra) : v];
                const uint32_t l = cw >> 16, nb = match ? l + eb + 1 : l;   // the distance code is one 0 bit
                tok[j] = (cw & 0xffff) | ((uint32_t)extra << l) | (nb << 24);
                nbits += nb;
            });
        }
        uint32_t incl = nbits;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < TPB / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (count > 0) {
            uint32_t pos = P - unit0 * 128 + before + incl - nbits;
            unsigned long long acc = 0;
            int fill = 0;
#pragma unroll
            for (int j = 0; j < RUN; ++j) {
                acc |= (unsigned long long)(tok[j] & 0xffffff) << fill;
                fill += tok[j] >> 24;
                if (fill >= 32) {
                    put_bits(buf, pos, acc & 0xffffffffull, 32);
                    pos += 32; acc >>= 32; fill -= 32;
                }
            }
            put_bits(buf, pos, acc, fill);
        }
        P += total;
        const bool tail = t0 + TILE > len;
        __syncthreads();
        if (tail && tid == 0) {
            const uint32_t e = code[EOB];
            put_bits(buf, P - unit0 * 128, e & 0xffff, e >> 16);
            P += e >> 16;
            if (!last) {
                P = ((P + 3 + 7) & ~7u) + 16;
                put_bits(buf, P - unit0 * 128, 0xffff, 16);
                P += 16;
            } else {
                P = (P + 7) & ~7u;
            }
            wsum[0] = P;
        }
        if (tail) {
            __syncthreads();
            P = wsum[0];
        }
        const uint32_t units = tail ? (P + 127) / 128 - unit0 : P / 128 - unit0;
        for (uint32_t u = tid; u < units; u += TPB)
            if ((long)(unit0 + u + 1) * 16 <= slot_cap) dst[unit0 + u] = reinterpret_cast<const uint4*>(buf)[u];   // (always: the chunk chose this block as the shorter one)
        if (tail) break;
        uint32_t keep = 0;
        if (tid < 4) keep = buf[units * 4 + tid];
        __syncthreads();
        for (int i = tid; i < RBUF_WORDS; i += TPB) buf[i] = 0;
        __syncthreads();
        if (tid < 4) buf[tid] = keep;
        unit0 += units;
        __syncthreads();
    }
}

}  // namespace

int ir_launch_png_encode_runs(const uint8_t* img, int n, int h, long pitch, int vh, int vw, uint8_t* out, size_t out_stride, uint32_t* info,
                              uint32_t* hist, uint32_t* codes, uint32_t* header, uint32_t* chunk_bytes, uint8_t* slots, long slot_cap,
                              uint32_t* run_hist, uint32_t* run_codes, uint32_t* run_header, uint32_t* flags, long flag_words, hipStream_t s) {
    Geo g;
    g.img = img; g.pitch = pitch; g.img_stride = (long)h * pitch; g.vh = vh; g.vw = vw; g.rowlen = 3 * vw + 1;
    g.chunks = (vh + ROWS - 1) / ROWS;
    if ((long)ROWS * g.rowlen > IR_PNG_RUNS_MAX_CHUNK)   // no room for a chunk's marks: every chunk literal-only
        return ir_launch_png_encode(img, n, h, pitch, vh, vw, out, out_stride, info, hist, codes, header, chunk_bytes, slots, slot_cap, s);
    const dim3 grid(g.chunks, n);
    hipLaunchKernelGGL(png_runs_hist_kernel, grid, dim3(TPB), 0, s, g, hist, run_hist, flags, flag_words);
    hipLaunchKernelGGL(png_codes_kernel, grid, dim3(64), 0, s, hist, codes, header, chunk_bytes, g.chunks);
    hipLaunchKernelGGL(png_runs_codes_kernel, grid, dim3(64), 0, s, run_hist, hist, codes, run_codes, run_header, chunk_bytes, g.chunks);
    hipLaunchKernelGGL(png_runs_encode_kernel, grid, dim3(TPB), 0, s, g, codes, header, slots, slot_cap, run_codes, run_header, flags, flag_words);
    hipLaunchKernelGGL(png_compact_kernel, grid, dim3(TPB), 0, s, slots, slot_cap, chunk_bytes, hist, out, out_stride, info, g.chunks, vh, g.rowlen);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int ir_launch_png_encode(const uint8_t* img, int n, int h, long pitch, int vh, int vw, uint8_t* out, size_t out_stride, uint32_t* info,
                         uint32_t* hist, uint32_t* codes, uint32_t* header, uint32_t* chunk_bytes, uint8_t* slots, long slot_cap, hipStream_t s) {
    Geo g;
    g.img = img; g.pitch = pitch; g.img_stride = (long)h * pitch; g.vh = vh; g.vw = vw; g.rowlen = 3 * vw + 1;
    g.chunks = (vh + ROWS - 1) / ROWS;
    const dim3 grid(g.chunks, n);
    hipLaunchKernelGGL(png_hist_kernel, grid, dim3(TPB), 0, s, g, hist);
    hipLaunchKernelGGL(png_codes_kernel, grid, dim3(64), 0, s, hist, codes, header, chunk_bytes, g.chunks);
    hipLaunchKernelGGL(png_encode_kernel, grid, dim3(TPB), 0, s, g, codes, header, slots, slot_cap);
    hipLaunchKernelGGL(png_compact_kernel, grid, dim3(TPB), 0, s, slots, slot_cap, chunk_bytes, hist, out, out_stride, info, g.chunks, vh, g.rowlen);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
