// Baseline JPEG encoding of uint8 HWC RGB device images (ir_jpeg_encode): per image the entropy-coded segment of one interleaved scan - what
// lies between the SOS header and EOI - with the standard (Annex K) Huffman tables and a restart interval. The host adds the headers
// (instarevive_amd/jpeg.py); tools/jpeg_encode_model.py is the definition, and the bytes equal libjpeg's. Integer arithmetic throughout.
//   coef     eight lanes per 8 x 8 block, blocks in the scan's order [image][MCU][block of the MCU]: libjpeg's RGB -> YCbCr (jccolor.c), for 4:2:0
//            chroma the h2v2 downsample with its alternating bias, jfdctint.c along the rows and down the columns, quantisation, int16
//            coefficients in zigzag order. Edge rule 1 is in the sampling: columns replicate the last full-resolution column, Y rows the last
//            row, full-resolution chroma rows only to an even count and then the last DOWNSAMPLED row replicates. Edge rule 2: a block of an MCU
//            outside the component's real grid (a dummy) has no AC and the DC of the previous block of its component in the MCU's order; its
//            lanes compute that block again and keep the DC, so no group waits for another.
//   code     one workgroup per restart interval, one wave per block and one lane per coefficient: the ballot of the non-zero lanes gives every
//            lane its run, a wave scan the bit offsets inside the block, a prefix over the tile's blocks the block's place; the lanes OR their
//            bits MSB-first into an LDS window whose finished 16-byte units go to the interval's slot. DC predictors chain inside the interval
//            only. Per interval: the byte count and the count of 0xFF bytes.
//   scan     one workgroup per image: the intervals' final offsets (stuffed size + the two marker bytes of every interval but the first), info.
//   compact  one workgroup per interval: FF D0+k, then the slot's bytes with 0x00 stuffed behind every 0xFF, at the final position.
// Four launches in stream order, because each consumes what other workgroups of the previous one produced (the per-XCD L2s are not coherent
// inside a launch).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int GROUPS = TPB / 8;              // 8 x 8 blocks per workgroup of the coefficient kernel
constexpr int PER_WAVE = 8;                  // blocks per wave and tile of the coder
constexpr int TILE = WAVES * PER_WAVE;       // blocks per tile
constexpr int BLOCK_BITS = IR_JPEG_BLOCK_BITS;
constexpr int BUF_WORDS = 4 + (TILE * BLOCK_BITS + 31) / 32 + 6;   // the carried 16-byte unit, a tile's bits at their worst, the pad; a multiple of 4
static_assert(BUF_WORDS % 4 == 0, "the window is flushed in 16-byte units");
constexpr int RUN = 16;                      // slot bytes per lane and tile of the compaction

struct Geo {
    const uint8_t* img;   // image 0, row 0
    long pitch, img_stride;
    int vh, vw;
    int s;                // 1: 4:4:4, 2: 4:2:0
    int mx, mcus, bpm;    // MCUs per row, MCUs per image, blocks per MCU
    int ry, rx;           // Y's real block grid
    int restart, intervals;
};

struct QTables {
    uint16_t t[2][64];   // luminance, chrominance; natural order
};

// ---------------------------------------------------------------- tables
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// per symbol: code | length << 16 (0 for a symbol the table does not have); [0 luminance, 1 chrominance]
struct HuffTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr void fill_codes(const HuffSpec& spec, uint32_t* out) {   // Annex C: canonical codes in order of length
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < spec.bits[l - 1]; ++i, ++k, ++code) out[spec.vals[k]] = code | ((uint32_t)l << 16);
        code <<= 1;
    }
}
constexpr HuffTables make_tables() {
    HuffTables t = {};
    fill_codes(DC_LUMA, t.dc[0]);
    fill_codes(DC_CHROMA, t.dc[1]);
    fill_codes(AC_LUMA, t.ac[0]);
    fill_codes(AC_CHROMA, t.ac[1]);
    return t;
}
__device__ const HuffTables g_huff = make_tables();

struct Zigzag {
    uint8_t at[64];   // position in zigzag order of natural index i
};
constexpr Zigzag make_zigzag() {
    constexpr uint8_t order[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    Zigzag z = {};
    for (int k = 0; k < 64; ++k) z.at[order[k]] = (uint8_t)k;
    return z;
}
__device__ const Zigzag g_zigzag = make_zigzag();

// ---------------------------------------------------------------- 1. coefficients
constexpr int FIX(double x) { return (int)(x * 65536.0 + 0.5); }

// component c (0 Y, 1 Cb, 2 Cr) of the pixel at p
IR_DEVINL int ycc(const uint8_t* __restrict__ p, int c) {
    const int r = p[0], g = p[1], b = p[2];
    if (c == 0) return (FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16;
    if (c == 1) return (-FIX(.16874) * r - FIX(.33126) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16;
    return (FIX(.5) * r - FIX(.41869) * g - FIX(.08131) * b + (128 << 16) + 32767) >> 16;
}

typedef long long i64;
constexpr i64 F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299, F_1_847 = 15137,
              F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
IR_DEVINL i64 descale(i64 x, int n) { return (x + ((i64)1 << (n - 1))) >> n; }

template <bool FIRST>
IR_DEVINL void fdct8(i64 d[8]) {   // jfdctint.c, one row (FIRST) or one column; as in degrade.hip
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    i64 t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const i64 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    i64 z1 = (t12 + t13) * F_0_541;
    d[2] = descale(z1 + t13 * F_0_765, N);
    d[6] = descale(z1 + t12 * (-F_1_847), N);
    z1 = t4 + t7;
    i64 z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const i64 z5 = (z3 + z4) * F_1_175;
    t4 *= F_0_298, t5 *= F_2_053, t6 *= F_3_072, t7 *= F_1_501;
    z1 *= -F_0_899, z2 *= -F_2_562, z3 *= -F_1_961, z4 *= -F_0_390;
    z3 += z5, z4 += z5;
    d[7] = descale(t4 + z1 + z3, N);
    d[5] = descale(t5 + z2 + z4, N);
    d[3] = descale(t6 + z2 + z3, N);
    d[1] = descale(t7 + z1 + z4, N);
}

// coef [image][MCU][block][64] int16, zigzag order; lane l of a group of eight takes row l, then column l of its block
__global__ __launch_bounds__(TPB) void jpeg_coef_kernel(Geo g, QTables qt, int16_t* __restrict__ coef) {
    __shared__ int s_c[GROUPS][8][9];
    __shared__ __attribute__((aligned(16))) int16_t s_z[GROUPS][64];
    const int l = threadIdx.x & 7, grp = threadIdx.x >> 3, image = blockIdx.y;
    const long per_image = (long)g.mcus * g.bpm;
    const long blk = (long)blockIdx.x * GROUPS + grp;
    const bool live = blk < per_image;
    const uint8_t* img = g.img + image * g.img_stride;
    const int ss = g.s * g.s;
    bool dummy = false;
    int comp = 0;
    i64 d[8];
    if (live) {
        const int m = (int)(blk / g.bpm), j = (int)(blk - (long)m * g.bpm);
        const int my = m / g.mx, mxi = m - my * g.mx;
        if (j < ss) {   // Y
            int by = my * g.s + j / g.s, bx = mxi * g.s + j % g.s;
            if (by >= g.ry) {   // a dummy row: the last real block of the MCU's first row
                dummy = true;
                by = my * g.s;
                bx = mxi * g.s + 1 < g.rx ? mxi * g.s + 1 : mxi * g.s;
            } else if (bx >= g.rx) {
                dummy = true;
                bx -= 1;
            }
            const int y = min(by * 8 + l, g.vh - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = ycc(img + (long)y * g.pitch + 3L * min(bx * 8 + i, g.vw - 1), 0) - 128;
        } else if (g.s == 1) {
            comp = 1 + j - ss;
            const int y = min(my * 8 + l, g.vh - 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = ycc(img + (long)y * g.pitch + 3L * min(mxi * 8 + i, g.vw - 1), comp) - 128;
        } else {
            comp = 1 + j - ss;
            const int ch = (g.vh + 1) >> 1, sy = min(my * 8 + l, ch - 1);   // rows past the true chroma height repeat the last DOWNSAMPLED row
            const uint8_t* ra = img + (long)(2 * sy) * g.pitch;
            const uint8_t* rb = img + (long)min(2 * sy + 1, g.vh - 1) * g.pitch;   // full-resolution rows replicate to an even count only
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int cx = mxi * 8 + i;
                const long xa = 3L * min(2 * cx, g.vw - 1), xb = 3L * min(2 * cx + 1, g.vw - 1);
                d[i] = ((ycc(ra + xa, comp) + ycc(ra + xb, comp) + ycc(rb + xa, comp) + ycc(rb + xb, comp) + 1 + (cx & 1)) >> 2) - 128;
            }
        }
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_c[grp][l][i] = (int)d[i];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_c[grp][i][l];
        fdct8<false>(d);   // the coefficients of column l, scaled by 8
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int Q = qt.t[comp ? 1 : 0][i * 8 + l], c = (int)d[i];
            const int m = ((c < 0 ? -c : c) + 4 * Q) / (8 * Q);
            s_z[grp][g_zigzag.at[i * 8 + l]] = (dummy && (i | l)) ? (int16_t)0 : (int16_t)(c < 0 ? -m : m);
        }
    }
    __syncthreads();
    if (live) reinterpret_cast<uint4*>(coef + ((long)image * per_image + blk) * 64)[l] = reinterpret_cast<const uint4*>(&s_z[grp][0])[l];
}

// ---------------------------------------------------------------- 2. entropy coding, one workgroup per restart interval
// OR the low n <= 32 bits of v into an LDS bit array at bit pos, MSB first (JPEG's order): bit 0 of the stream is bit 31 of word 0
IR_DEVINL void put_bits(uint32_t* buf, uint32_t pos, uint32_t v, int n) {
    if (!n) return;
    const uint32_t w = pos >> 5, sh = pos & 31;
    const unsigned long long x = (unsigned long long)v << (64 - sh - n);
    atomicOr(&buf[w], (uint32_t)(x >> 32));
    if (sh + n > 32) atomicOr(&buf[w + 1], (uint32_t)x);
}

struct Token {
    uint32_t val;   // Huffman code and value bits
    int len, zrl;   // their bit count; ZRL symbols in front of them
};

// What lane k writes for its coefficient c of zigzag position k (lane 0: the DC difference); nz: the ballot of the non-zero AC lanes.
// Sizes beyond what 8-bit samples can give (11 for DC, 10 for AC) are cut, which keeps a block inside IR_JPEG_BLOCK_BITS whatever it holds.
IR_DEVINL Token make_token(int c, int lane, unsigned long long nz, const uint32_t* __restrict__ dc, const uint32_t* __restrict__ ac) {
    Token t = {0, 0, 0};
    const int a = c < 0 ? -c : c;
    int size = 32 - __clz(a);
    if (lane == 0) {
        size = min(size, 11);
        const uint32_t e = dc[size];
        t.val = ((e & 0xffff) << size) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1));
        t.len = (int)(e >> 16) + size;
    } else if (c != 0) {
        size = min(size, 10);
        const unsigned long long lower = nz & ((1ull << lane) - 1);
        const int prev = lower ? 63 - __clzll((long long)lower) : 0;
        const int run = lane - prev - 1;
        const uint32_t e = ac[((run & 15) << 4) | size];
        t.zrl = run >> 4;
        t.val = ((e & 0xffff) << size) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1));
        t.len = (int)(e >> 16) + size;
    } else if (lane == 63) {   // the block ends in zeros: EOB
        t.val = ac[0] & 0xffff;
        t.len = (int)(ac[0] >> 16);
    }
    return t;
}

// slots [image * intervals + interval][slot_cap]: the interval's bytes before stuffing, in whole 16-byte units; raw: their count; ffs: the 0xFF among them
__global__ __launch_bounds__(TPB) void jpeg_code_kernel(Geo g, const int16_t* __restrict__ coef, uint8_t* __restrict__ slots, long slot_cap,
                                                        uint32_t* __restrict__ raw, uint32_t* __restrict__ ffs) {
    __shared__ uint32_t s_dc[2][16], s_ac[2][256];
    __shared__ __attribute__((aligned(16))) uint32_t buf[BUF_WORDS];
    __shared__ uint32_t blk_bits[TILE];
    __shared__ uint32_t s_ff;
    const int interval = blockIdx.x, image = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slot = (long)image * g.intervals + interval;
    const int mcu0 = interval * g.restart;
    const int nblk = min(g.restart, g.mcus - mcu0) * g.bpm;
    const int16_t* src = coef + ((long)image * g.mcus + mcu0) * g.bpm * 64;
    uint4* dst = reinterpret_cast<uint4*>(slots + slot * slot_cap);
    const int ss = g.s * g.s;
    for (int i = tid; i < 2 * 16; i += TPB) (&s_dc[0][0])[i] = (&g_huff.dc[0][0])[i];
    for (int i = tid; i < 2 * 256; i += TPB) (&s_ac[0][0])[i] = (&g_huff.ac[0][0])[i];
    for (int i = tid; i < BUF_WORDS; i += TPB) buf[i] = 0;
    if (tid == 0) s_ff = 0;
    __syncthreads();
    uint32_t P = 0;        // bits of the interval so far
    uint32_t unit0 = 0;    // 16-byte units already stored; the window starts at bit unit0 * 128
    uint32_t ff = 0;
    for (int t0 = 0; t0 < nblk; t0 += TILE) {
        int c[PER_WAVE];
        uint32_t off[PER_WAVE];
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int b = t0 + wave * PER_WAVE + i;
            c[i] = b < nblk ? (int)src[(long)b * 64 + lane] : 0;
        }
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int b = t0 + wave * PER_WAVE + i;   // wave-uniform
            uint32_t bits = 0;
            if (b < nblk) {
                const int m = b / g.bpm, j = b - m * g.bpm;
                if (lane == 0) {   // the DC difference against the previous block of the component inside the interval
                    const int back = j < ss ? (j > 0 ? 1 : g.bpm - ss + 1) : g.bpm;
                    if (b - back >= 0 && (m > 0 || (j > 0 && j < ss))) c[i] -= (int)src[(long)(b - back) * 64];
                }
                const int tab = j < ss ? 0 : 1;
                const unsigned long long nz = __ballot(c[i] != 0 && lane > 0);
                const Token t = make_token(c[i], lane, nz, s_dc[tab], s_ac[tab]);
                bits = (uint32_t)(t.len + t.zrl * (int)(s_ac[tab][0xF0] >> 16));
            }
            uint32_t incl = bits;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            off[i] = incl - bits;
            if (lane == 63) blk_bits[wave * PER_WAVE + i] = incl;
        }
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int k = 0; k < TILE; ++k) {
            if (k < wave * PER_WAVE) before += blk_bits[k];
            total += blk_bits[k];
        }
        uint32_t at = P - unit0 * 128 + before;
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const int b = t0 + wave * PER_WAVE + i;
            if (b < nblk) {
                const int j = b % g.bpm, tab = j < ss ? 0 : 1;
                const unsigned long long nz = __ballot(c[i] != 0 && lane > 0);
                const Token t = make_token(c[i], lane, nz, s_dc[tab], s_ac[tab]);
                const uint32_t z = s_ac[tab][0xF0];
                uint32_t pos = at + off[i];
                for (int k = 0; k < t.zrl; ++k) {
                    put_bits(buf, pos, z & 0xffff, (int)(z >> 16));
                    pos += z >> 16;
                }
                put_bits(buf, pos, t.val, t.len);
            }
            at += blk_bits[wave * PER_WAVE + i];
        }
        P += total;
        const bool tail = t0 + TILE >= nblk;
        if (tail) {   // pad the last byte with 1-bits (every thread knows P)
            const int pad = (int)((8 - (P & 7)) & 7);
            if (tid == 0) put_bits(buf, P - unit0 * 128, (1u << pad) - 1, pad);
            P += pad;
        }
        __syncthreads();
        const uint32_t units = (tail ? (P + 127) / 128 : P / 128) - unit0;   // the tail stores its partial unit too (zero padded, inside the slot)
        for (uint32_t u = tid; u < units; u += TPB) {
            uint4 v = reinterpret_cast<const uint4*>(buf)[u];
            ff += ((v.x >> 24) == 0xff) + (((v.x >> 16) & 0xff) == 0xff) + (((v.x >> 8) & 0xff) == 0xff) + ((v.x & 0xff) == 0xff);
            ff += ((v.y >> 24) == 0xff) + (((v.y >> 16) & 0xff) == 0xff) + (((v.y >> 8) & 0xff) == 0xff) + ((v.y & 0xff) == 0xff);
            ff += ((v.z >> 24) == 0xff) + (((v.z >> 16) & 0xff) == 0xff) + (((v.z >> 8) & 0xff) == 0xff) + ((v.z & 0xff) == 0xff);
            ff += ((v.w >> 24) == 0xff) + (((v.w >> 16) & 0xff) == 0xff) + (((v.w >> 8) & 0xff) == 0xff) + ((v.w & 0xff) == 0xff);
            v.x = __builtin_bswap32(v.x); v.y = __builtin_bswap32(v.y); v.z = __builtin_bswap32(v.z); v.w = __builtin_bswap32(v.w);   // to byte order
            dst[unit0 + u] = v;
        }
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
    for (int o = 32; o > 0; o >>= 1) ff += __shfl_down(ff, o, 64);
    if (lane == 0) atomicAdd(&s_ff, ff);
    __syncthreads();
    if (tid == 0) {
        raw[slot] = P / 8;
        ffs[slot] = s_ff;
    }
}

// inclusive sum over the workgroup's threads; `total` gets the sum of all
IR_DEVINL uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    __syncthreads();   // (the previous call's readers are done with wsum)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    total = 0;
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) incl += wsum[w];
        total += wsum[w];
    }
    return incl;
}

// ---------------------------------------------------------------- 3. the intervals' places, one workgroup per image
__global__ __launch_bounds__(TPB) void jpeg_scan_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ ffs, uint32_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ info, int intervals) {
    __shared__ uint32_t wsum[WAVES];
    const int image = blockIdx.x, tid = threadIdx.x;
    const long base = (long)image * intervals;
    uint32_t carry = 0;
    for (int t0 = 0; t0 < intervals; t0 += TPB) {
        const int i = t0 + tid;
        const uint32_t v = i < intervals ? raw[base + i] + ffs[base + i] + (i > 0 ? 2u : 0u) : 0u;
        uint32_t total;
        const uint32_t incl = block_scan(v, wsum, total);
        if (i < intervals) offsets[base + i] = carry + incl - v;
        carry += total;
    }
    if (tid == 0) info[image] = carry;
}

// ---------------------------------------------------------------- 4. compaction with stuffing and markers, one workgroup per interval
__global__ __launch_bounds__(TPB) void jpeg_compact_kernel(const uint8_t* __restrict__ slots, long slot_cap, const uint32_t* __restrict__ raw,
                                                           const uint32_t* __restrict__ offsets, uint8_t* __restrict__ out, size_t out_stride, int intervals) {
    __shared__ uint32_t wsum[WAVES];
    const int interval = blockIdx.x, image = blockIdx.y, tid = threadIdx.x;
    const long slot = (long)image * intervals + interval;
    const uint32_t nbytes = raw[slot];
    const uint4* src = reinterpret_cast<const uint4*>(slots + slot * slot_cap);   // 16-byte aligned, stored in whole units
    uint8_t* dst = out + (size_t)image * out_stride + offsets[slot];
    if (interval > 0) {
        if (tid == 0) {
            dst[0] = 0xff;
            dst[1] = (uint8_t)(0xd0 + ((interval - 1) & 7));
        }
        dst += 2;
    }
    uint32_t done = 0;   // stuffed bytes written by the tiles so far
    for (uint32_t t0 = 0; t0 < nbytes; t0 += TPB * RUN) {
        const uint32_t k0 = t0 + tid * RUN;
        const int count = k0 < nbytes ? (int)min((uint32_t)RUN, nbytes - k0) : 0;
        uint4 v = {0, 0, 0, 0};
        if (count > 0) v = src[k0 / RUN];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < RUN; ++j) mine += (j < count && ((w[j >> 2] >> (8 * (j & 3))) & 0xff) == 0xff) ? 2u : (j < count ? 1u : 0u);
        uint32_t total;
        const uint32_t incl = block_scan(mine, wsum, total);
        uint8_t* o = dst + done + incl - mine;
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (j < count) {
                const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
                *o++ = (uint8_t)b;
                if (b == 0xff) *o++ = 0;
            }
        done += total;
    }
}

}  // namespace

// blocks per MCU and MCUs of a vh x vw image; false for a subsampling the encoder does not have
static bool jpeg_geometry(int vh, int vw, int subsampling, int* s, long* mx, long* my) {
    if (subsampling != 0 && subsampling != 2) return false;
    *s = subsampling == 2 ? 2 : 1;
    *mx = ((long)vw + 8 * *s - 1) / (8 * *s);
    *my = ((long)vh + 8 * *s - 1) / (8 * *s);
    return true;
}

size_t ir_jpeg_bound_host(int h, int w, int subsampling, int restart_mcus) {
    int s;
    long mx, my;
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || restart_mcus < 1 || restart_mcus > 65535 || !jpeg_geometry(h, w, subsampling, &s, &mx, &my)) return 0;
    const size_t mcus = (size_t)mx * my, blocks = mcus * (s * s + 2), intervals = (mcus + restart_mcus - 1) / restart_mcus;
    // every interval rounds its bits up to a byte; stuffing at most doubles the bytes; two marker bytes per interval
    return 2 * ((blocks * IR_JPEG_BLOCK_BITS + 7) / 8 + intervals) + 2 * intervals;
}

bool ir_jpeg_layout(int n, int vh, int vw, int subsampling, int restart_mcus, IrJpegLayout* L) {
    int s;
    long mx, my;
    const size_t bound = ir_jpeg_bound_host(vh, vw, subsampling, restart_mcus);
    if (n < 1 || n > 65535 || !bound || bound > 0xffffffffu || !jpeg_geometry(vh, vw, subsampling, &s, &mx, &my)) return false;
    const size_t mcus = (size_t)mx * my, bpm = s * s + 2, intervals = (mcus + restart_mcus - 1) / restart_mcus;
    const size_t most = std::min<size_t>(restart_mcus, mcus) * bpm;   // blocks of the longest interval
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t k = (size_t)n * intervals;
    if (k > 0x7fffffffu) return false;
    L->intervals = intervals;
    L->slot_cap = (((most * IR_JPEG_BLOCK_BITS + 7) / 8 + 15) & ~(size_t)15) + 16;   // stored in whole 16-byte units
    L->coef = 0;
    L->raw = L->coef + up((size_t)n * mcus * bpm * 64 * sizeof(int16_t));
    L->ffs = L->raw + up(k * 4);
    L->offsets = L->ffs + up(k * 4);
    L->slots = L->offsets + up(k * 4);
    L->total = L->slots + up(k * L->slot_cap);
    return true;
}

int ir_launch_jpeg_encode(const uint8_t* img, int n, int h, long pitch, int vh, int vw, int quality, int subsampling, int restart_mcus, uint8_t* out,
                          size_t out_stride, uint32_t* info, void* ws, hipStream_t stream) {
    IrJpegLayout L;
    int s;
    long mx, my;
    if (quality < 1 || quality > 100 || !ir_jpeg_layout(n, vh, vw, subsampling, restart_mcus, &L) || !jpeg_geometry(vh, vw, subsampling, &s, &mx, &my)) return -1;
    Geo g;
    g.img = img; g.pitch = pitch; g.img_stride = (long)h * pitch; g.vh = vh; g.vw = vw; g.s = s;
    g.mx = (int)mx; g.mcus = (int)(mx * my); g.bpm = s * s + 2;
    g.ry = (vh + 7) / 8; g.rx = (vw + 7) / 8;
    g.restart = restart_mcus; g.intervals = (int)L.intervals;
    QTables qt;
    ir_degrade_qtables_host(quality, qt.t[0], qt.t[1]);
    char* b = static_cast<char*>(ws);
    int16_t* coef = reinterpret_cast<int16_t*>(b + L.coef);
    uint32_t *raw = reinterpret_cast<uint32_t*>(b + L.raw), *ffs = reinterpret_cast<uint32_t*>(b + L.ffs), *offsets = reinterpret_cast<uint32_t*>(b + L.offsets);
    uint8_t* slots = reinterpret_cast<uint8_t*>(b + L.slots);
    const long blocks = (long)g.mcus * g.bpm;
    const dim3 per_interval(g.intervals, n);
    hipLaunchKernelGGL(jpeg_coef_kernel, dim3((unsigned)((blocks + GROUPS - 1) / GROUPS), n), dim3(TPB), 0, stream, g, qt, coef);
    hipLaunchKernelGGL(jpeg_code_kernel, per_interval, dim3(TPB), 0, stream, g, coef, slots, (long)L.slot_cap, raw, ffs);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(TPB), 0, stream, raw, ffs, offsets, info, g.intervals);
    hipLaunchKernelGGL(jpeg_compact_kernel, per_interval, dim3(TPB), 0, stream, slots, (long)L.slot_cap, raw, offsets, out, out_stride, g.intervals);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
