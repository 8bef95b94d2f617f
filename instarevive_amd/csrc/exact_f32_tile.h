// The exact-fp32 tile loop of the metric models: lpips_conv_kernel, dists_conv_kernel, fid_conv_kernel, clipiqa_conv_kernel, musiq_gemm_kernel and
// maniqa_gemm_kernel are this one loop with their own operands and epilogue.
//   C[M][N] = A[M][K] B[K][N] on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain from 0, so an output element
//   depends neither on the tile it falls in nor on its place in a batch). A workgroup of four waves owns a BM x BN tile, WM x WN waves with
//   WN = 2 from BN = 64 on, a wave TM x TN blocks of 32 x 32. The 32-deep k-tile goes global -> registers -> LDS (s_a[32][BM + 4], s_b[32][BN + 4],
//   k-major, so an MFMA operand is one conflict-free LDS read per lane) with the next tile's loads in flight during the MFMAs; the two
//   __syncthreads() of a k-tile are the only barriers. The column of an accumulator element is on the lane, so a row of the tile is one
//   128-byte store per wave. No floating-point atomics: the same bits on every call.
//   Operands at or behind M, N, K read as exact zeros (fmaf(0, 0, acc) = acc); every store is guarded by M, and by N where N is no tile multiple.
// An operand is a struct with rows(first row / column of the tile), load(k0) - issue the global loads of k-tile k0 into its own registers - and
// store(LDS tile); an epilogue has column(col) -> is the column live (it fetches what belongs to the column) and store(m, acc). All state is held
// by value and every member is IR_DEVINL, so the policies dissolve into the kernel's registers.
// A kernel states in its __launch_bounds__ the waves per SIMD its tile is built for: with that bound the compiler keeps the accumulators in
// VGPRs beside the operands' registers, uses no scratch and holds that occupancy; without it the registers of the tile in flight go to scratch.
// THE LOOP AND THE OPERANDS HOLD NO FLOATING-POINT ARITHMETIC but the MFMA: lpips.hip is built with -ffp-contract=fast and the other five
// with -ffp-contract=off, so whatever rounds - the epilogues, the input tables - is written in the including file under that file's flag.
#pragma once
#include "common.h"

namespace exact_tile {

constexpr int TPB = 256;   // four waves
constexpr int BK = 32;     // depth of a k-tile

// The A tile from a thread's float4 of four k (4 * (tid & 7) ..) for the rows (tid >> 3) + 32 i
template <int AR, int LDA>
IR_DEVINL void store_a_k4(float (&s_a)[BK][LDA], const float4 (&gv)[AR]) {
    const int tid = threadIdx.x, kq = 4 * (tid & 7);
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        const int row = (tid >> 3) + 32 * i;
        s_a[kq][row] = gv[i].x;
        s_a[kq + 1][row] = gv[i].y;
        s_a[kq + 2][row] = gv[i].z;
        s_a[kq + 3][row] = gv[i].w;
    }
}
// ... and from a thread's scalars of one k (tid & 31) for the rows (tid >> 5) + 8 i
template <int AR, int LDA>
IR_DEVINL void store_a_k1(float (&s_a)[BK][LDA], const float (&ga)[AR]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < AR; ++i) s_a[tid & 31][(tid >> 5) + 8 * i] = ga[i];
}

// A: the implicit im2col of a kh x kw conv over NHWC fp32 maps [imgs][H][W][pitch] (the first cin channels; cin a multiple of 4), K = kh kw cin
// in (ky, kx, c) order. TILE_TAP: cin is a multiple of BK, so a k-tile never crosses a tap and K has no tail - the tap is computed once per
// tile; else every thread's float4 has its own tap and is guarded by k < K. A row at or behind M has riy = -2^20: every tap out of bounds.
template <int BM, bool TILE_TAP>
struct NhwcA {
    static constexpr int AR = BM * BK / 4 / TPB;
    const float* in;
    int H, W, cin, pitch, kw, stride, ph, pw, Ho, Wo, M, K;
    long ro[AR];   // the offset of tap (0, 0)'s pixel
    int riy[AR], rix[AR];
    float4 gv[AR];

    IR_DEVINL void rows(int m0) {
        const int HWo = Ho * Wo;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + ((int)threadIdx.x >> 3) + 32 * i;
            if (m < M) {
                const int img = m / HWo, r = m - img * HWo, oy = r / Wo, ox = r - oy * Wo;
                riy[i] = oy * stride - ph;
                rix[i] = ox * stride - pw;
                ro[i] = (((long)img * H + riy[i]) * W + rix[i]) * pitch;
            } else {
                riy[i] = -(1 << 20);
                rix[i] = 0;
                ro[i] = 0;
            }
        }
    }
    IR_DEVINL void load(int k0) {
        const int kq = 4 * ((int)threadIdx.x & 7), k = TILE_TAP ? k0 : k0 + kq;
        const int tap = k / cin, c0 = k - tap * cin + (TILE_TAP ? kq : 0);
        const int ky = tap / kw, kx = tap - ky * kw;
        const long toff = ((long)ky * W + kx) * pitch + c0;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int iy = riy[i] + ky, ix = rix[i] + kx;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((TILE_TAP || k < K) && iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const float4*>(in + ro[i] + toff);
            gv[i] = v;
        }
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const { store_a_k4(s_a, gv); }
};

// A: the implicit im2col of a conv over RGB8 byte images through a 3 x 256 table (channel, byte) -> fp32, which rows() copies to LDS (s_tab,
// the kernel's) and ends with the barrier that publishes it. K = rows x row_k with row_k = 3 x (taps of one image row) in (ky, kx, c) order,
// guarded by k < K; padding is 0 in the table's domain. TWO: images n .. come from a second buffer b with its own pitch.
template <int BM, bool TWO>
struct ByteTableA {
    static constexpr int AR = BM * BK / TPB;
    const uint8_t *a, *b;
    long a_pitch, a_img, b_pitch, b_img;
    int n;
    const float* tab;
    float* s_tab;
    int H, W, Ho, Wo, row_k, stride, pad, M, K;
    const uint8_t* rb[AR];
    int riy[AR], rix[AR];
    bool rsec[TWO ? AR : 1];   // the row belongs to an image of b
    float ga[AR];

    IR_DEVINL void rows(int m0) {
        const int tid = threadIdx.x, HWo = Ho * Wo;
        for (int i = tid; i < 3 * 256; i += TPB) s_tab[i] = tab[i];
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + (tid >> 5) + 8 * i;
            if (m < M) {
                const int img = m / HWo, r = m - img * HWo, oy = r / Wo, ox = r - oy * Wo;
                const bool sec = TWO && img >= n;
                riy[i] = oy * stride - pad;
                rix[i] = ox * stride - pad;
                rb[i] = sec ? b + (long)(img - n) * b_img : a + (long)img * a_img;
                rb[i] += (long)riy[i] * (sec ? b_pitch : a_pitch) + 3L * rix[i];
                if constexpr (TWO) rsec[i] = sec;
            } else {
                riy[i] = -(1 << 20);
                rix[i] = 0;
                rb[i] = a;
                if constexpr (TWO) rsec[i] = false;
            }
        }
        __syncthreads();
    }
    IR_DEVINL void load(int k0) {
        const int k = k0 + ((int)threadIdx.x & 31);
        const int ky = k / row_k, r = k - ky * row_k, kx = r / 3, c = r - kx * 3;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int iy = riy[i] + ky, ix = rix[i] + kx;
            float v = 0.f;
            if (k < K && iy >= 0 && iy < H && ix >= 0 && ix < W) v = s_tab[256 * c + rb[i][(long)ky * (TWO && rsec[i] ? b_pitch : a_pitch) + r]];
            ga[i] = v;
        }
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const { store_a_k1(s_a, ga); }
};

// A: row-major rows [M][lda], lda and K multiples of 4. KGUARD: K is no multiple of BK, a float4 at or behind it reads as zero.
template <int BM, bool KGUARD>
struct RowsA {
    static constexpr int AR = BM * BK / 4 / TPB;
    const float* a;
    long lda;
    int M, K;
    long ro[AR];
    float4 gv[AR];

    IR_DEVINL void rows(int m0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + ((int)threadIdx.x >> 3) + 32 * i;
            ro[i] = m < M ? (long)m * lda : -1;
        }
    }
    IR_DEVINL void load(int k0) {
        const int k = k0 + 4 * ((int)threadIdx.x & 7);
#pragma unroll
        for (int i = 0; i < AR; ++i) gv[i] = (ro[i] >= 0 && (!KGUARD || k < K)) ? *reinterpret_cast<const float4*>(a + ro[i] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const { store_a_k4(s_a, gv); }
};

// B as [K][ldb]. GUARD false: the repacked conv weights - rows up to K rounded up to BK exist, ldb is a multiple of BN; true: rows at or behind
// Kb and columns at or behind N read as zero.
template <int BN, bool GUARD>
struct KnB {
    static constexpr int BV = BK * BN / 4 / TPB;
    const float* b;
    long ldb;
    int Kb, N;
    int n0;
    float4 gb[BV];

    IR_DEVINL void rows(int n) { n0 = n; }
    IR_DEVINL void load(int k0) {
        const float* tile = b + (long)k0 * ldb + n0;   // uniform; a thread's offsets inside the tile are ints that do not change from tile to tile
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, kr = idx / (BN / 4), nc = idx - kr * (BN / 4);
            gb[i] = (!GUARD || (k0 + kr < Kb && n0 + 4 * nc < N)) ? *reinterpret_cast<const float4*>(tile + (kr * (int)ldb + 4 * nc)) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    template <int LDB>
    IR_DEVINL void store(float (&s_b)[BK][LDB]) const {
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, kr = idx / (BN / 4), nc = idx - kr * (BN / 4);
            *reinterpret_cast<float4*>(&s_b[kr][4 * nc]) = gb[i];
        }
    }
};

// B as [N][ldb] (the K of Q K^T): rows at or behind N read as zero; KGUARD: so does a float4 at or behind K.
template <int BN, bool KGUARD>
struct NkB {
    static constexpr int BV = BK * BN / 4 / TPB;
    const float* b;
    long ldb;
    int N, K;
    int n0;
    float4 gb[BV];

    IR_DEVINL void rows(int n) { n0 = n; }
    IR_DEVINL void load(int k0) {
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, row = idx >> 3, kq = 4 * (idx & 7);
            gb[i] = (n0 + row < N && (!KGUARD || k0 + kq < K)) ? *reinterpret_cast<const float4*>(b + (long)(n0 + row) * ldb + k0 + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    template <int LDB>
    IR_DEVINL void store(float (&s_b)[BK][LDB]) const {
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, row = idx >> 3, kq = 4 * (idx & 7);
            s_b[kq][row] = gb[i].x;
            s_b[kq + 1][row] = gb[i].y;
            s_b[kq + 2][row] = gb[i].z;
            s_b[kq + 3][row] = gb[i].w;
        }
    }
};

// The tile blockIdx.x, blockIdx.y of C: K in k-tiles through a and b, then every accumulator element (m, col) with m < M of a live column to epi.
template <int BM, int BN, class AOp, class BOp, class Epi>
IR_DEVINL void tile_loop(AOp a, BOp b, int M, int K, Epi epi) {
    constexpr int WN = BN >= 64 ? 2 : 1, WM = 4 / WN;         // waves across the tile
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);   // 32 x 32 blocks per wave
    static_assert(TM >= 1 && TN >= 1 && BK * BN / 4 >= TPB, "tile too small for four waves");
    __shared__ __attribute__((aligned(16))) float s_a[BK][BM + 4];
    __shared__ __attribute__((aligned(16))) float s_b[BK][BN + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int nk = (K + BK - 1) / BK;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    a.rows(m0);
    b.rows(n0);
    a.load(0);
    b.load(0);
    const int kh = lane >> 5, l31 = lane & 31;
    for (int kt = 0; kt < nk; ++kt) {
        a.store(s_a);
        b.store(s_b);
        __syncthreads();
        if (kt + 1 < nk) {
            a.load((kt + 1) * BK);
            b.load((kt + 1) * BK);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = s_a[kk + kh][wm * (32 * TM) + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = s_b[kk + kh][wn * (32 * TN) + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (32 * TN) + j * 32 + l31;
        if (!epi.column(col)) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * (32 * TM) + i * 32 + mfma_row(r, lane);
                if (m < M) epi.store(m, acc[i][j][r]);
            }
    }
}

}  // namespace exact_tile
