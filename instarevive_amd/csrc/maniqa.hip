// MANIQA of uint8 HWC RGB device images (ir_maniqa): the model of tools/evaluate_maniqa.py - `crops` windows of crop x crop pixels per image at
// given origins, a ViT trunk of which four block outputs are tapped, two transposed-attention blocks (TAB) and a Swin stage, twice, two small
// heads per patch token and one weighted mean over the patches of all crops of an image - in exact fp32 with fp64 statistics.
//   Contractions: ONE GEMM kernel on the exact-fp32 tile loop of exact_f32_tile.h (an output element depends neither on the tile it falls in, nor
//   on the crop's place in a launch, nor on the image's place in a batch), 128 x 64 tiles. The A operand is row-major rows, k-major columns (A[k][m]: the 1 x 1 convs read the [C][N] maps as they
//   lie), or the implicit im2col of the patch conv straight from the byte image through the 256-entry table at a crop's origin - no crop is ever
//   materialised as pixels; the origin is clamped into the scored rectangle, so every read stays inside it. The B operand is [K][N] or [N][K].
//   K need not be a multiple of the k-tile (N = 784 tokens): operands at or behind K read as exact zeros, as do the padded key columns of the
//   ViT's probabilities. Epilogue: acc * alpha + bias[col] + residual, separate roundings (the file is built with -ffp-contract=off); the TAB's
//   P V stores element [c][n] at n * C + c - the published reinterpretation - and adds the residual read at that same address of the INPUT map;
//   the output is another buffer, so no residual is overwritten before it is read.
//   Window attention (16 tokens, below any MFMA tile in M): a dedicated kernel, one wave per (crop, window, head). The window's tokens are the
//   rows 0 .. 15 of one 32 x 32 MFMA tile (the other rows and columns are fed zeros), gathered by index arithmetic from the cyclically shifted
//   grid; q is scaled before the chain as the published code does; the relative-position bias and the -100 mask of the shifted windows' region
//   labels are added in the softmax, which runs per row in fp64 in key order.
//   The heads' last linear and the pooled sum: fp64, each a per-lane sequential chain followed by a fixed fold; LayerNorm, softmax rows and the
//   exact GELU are the kernels of exact_rows.h. The crops of a call are processed in passes of as many crops as the workspace holds; the
//   per-patch (s, w) of every crop are kept, and ONE reduction per image makes the score, whose bits thus do not depend on the passes.
// Every store is guarded by the element count of its launch.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "exact_f32_tile.h"
#include "exact_rows.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int BM = 128, BN = 64;
constexpr size_t SCORE_BYTES = (size_t)1 << 26;   // the ViT score matrices of one attention launch: as many (crop, head) pairs as fit, at least one

enum { A_ROWS = 0, A_KM = 1, A_PATCH = 2 };
enum { B_KN = 0, B_NK = 1 };

struct GemmArgs {
    const float* a;   // A_ROWS: [M][lda]; A_KM: [K][lda]
    long lda;
    const float* b;   // B_KN: [K][ldb], B_NK: [N][ldb]
    long ldb;
    int Kb;           // B_KN: rows at or behind it read as zero
    int M, N, K;      // operands at or behind K read as zero; K a multiple of 4 (A_ROWS, B_NK)
    const float *bias, *res;   // [N] / addressed as c, or null
    float alpha;
    float* c;
    long ldc;
    int tstore;       // element (m, col) lies at col * ldc + m instead of m * ldc + col (c and res)
    // grid.z: pair z0 + blockIdx.z is (crop, head) = (pair / zdiv, pair % zdiv); an operand moves by s0 per crop, s1 per head, sl per blockIdx.z
    int z0, zdiv;
    long a_s0, a_s1, a_sl, b_s0, b_s1, b_sl, c_s0, c_s1, c_sl, r_s0;
    // A_PATCH: row m is patch token m % tokens of crop g0 + m / tokens, k is (channel, ky, kx)
    const uint8_t* img;
    long pitch, img_stride;
    const int* origins;   // [..][2]: y, x
    const float* tab;
    int g0, crops, h, w, crop, patch, G;
};

// A_KM: k-major columns A[k][m] (the 1 x 1 convs read the [C][N] maps as they lie): the tile is copied as it lies, zeros at or behind K and M
struct KmA {
    static constexpr int AR = BM * BK / 4 / TPB;
    const float* a;
    long lda;
    int M, K;
    int m0;
    float4 gv[AR];

    IR_DEVINL void rows(int m) { m0 = m; }
    IR_DEVINL void load(int k0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, kr = idx / (BM / 4), mc = idx - kr * (BM / 4);
            gv[i] = (k0 + kr < K && m0 + 4 * mc < M) ? *reinterpret_cast<const float4*>(a + (long)(k0 + kr) * lda + m0 + 4 * mc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int idx = (int)threadIdx.x + i * TPB, kr = idx / (BM / 4), mc = idx - kr * (BM / 4);
            *reinterpret_cast<float4*>(&s_a[kr][4 * mc]) = gv[i];
        }
    }
};

// A_PATCH: the implicit im2col of the patch conv from the byte image through the 256-entry table; row m is patch token m % tokens of crop
// g0 + m / tokens at its origin (clamped into the scored rectangle), k is (channel, ky, kx)
struct PatchA {
    static constexpr int AR = BM * BK / TPB;
    const GemmArgs& p;
    long ro[AR];
    float ga[AR];

    IR_DEVINL void rows(int m0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + ((int)threadIdx.x >> 5) + 8 * i;
            ro[i] = -1;
            if (m < p.M) {
                const int tokens = p.G * p.G, lc = m / tokens, t = m - lc * tokens, gy = t / p.G, gx = t - gy * p.G;
                const long g = (long)p.g0 + lc;
                const int oy = min(max(p.origins[2 * g], 0), p.h - p.crop), ox = min(max(p.origins[2 * g + 1], 0), p.w - p.crop);
                ro[i] = (g / p.crops) * p.img_stride + (long)(oy + gy * p.patch) * p.pitch + 3L * (ox + gx * p.patch);
            }
        }
    }
    IR_DEVINL void load(int k0) {
        const int k = k0 + ((int)threadIdx.x & 31), pp = p.patch * p.patch;
        const int ch = k / pp, r = k - ch * pp, ky = r / p.patch, kx = r - ky * p.patch;
        const long ko = (long)ky * p.pitch + 3L * kx + ch;
#pragma unroll
        for (int i = 0; i < AR; ++i) ga[i] = (k < p.K && ro[i] >= 0) ? p.tab[p.img[ro[i] + ko]] : 0.f;
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const { store_a_k1(s_a, ga); }
};

// acc * alpha + bias[col] + residual, separate roundings; tstore: element (m, col) lies at col * ldc + m (c and the residual)
struct AlphaBiasRes {
    const GemmArgs& p;
    float* c;
    const float* res;
    int col;
    float bs;
    IR_DEVINL bool column(int n) {
        if (n >= p.N) return false;
        col = n;
        bs = p.bias ? p.bias[n] : 0.f;
        return true;
    }
    IR_DEVINL void store(int m, float acc) const {
        const long at = p.tstore ? (long)col * p.ldc + m : (long)m * p.ldc + col;
        float v = acc * p.alpha;
        v = v + bs;
        if (res) v = v + res[at];
        c[at] = v;
    }
};

template <int AMODE, int BMODE>
__global__ __launch_bounds__(TPB, AMODE == A_PATCH ? 3 : AMODE == A_KM ? 5 : 4) void maniqa_gemm_kernel(GemmArgs p) {
    const int pair = p.z0 + (int)blockIdx.z, zi = pair / p.zdiv, zj = pair - zi * p.zdiv;
    const float* A = AMODE == A_PATCH ? nullptr : p.a + zi * p.a_s0 + zj * p.a_s1 + (long)blockIdx.z * p.a_sl;
    const float* B = p.b + zi * p.b_s0 + zj * p.b_s1 + (long)blockIdx.z * p.b_sl;
    const AlphaBiasRes epi{p, p.c + zi * p.c_s0 + zj * p.c_s1 + (long)blockIdx.z * p.c_sl, p.res ? p.res + zi * p.r_s0 : nullptr};
    const auto run = [&](auto a) {
        if constexpr (BMODE == B_KN)
            tile_loop<BM, BN>(a, KnB<BN, true>{.b = B, .ldb = p.ldb, .Kb = p.Kb, .N = p.N}, p.M, p.K, epi);
        else
            tile_loop<BM, BN>(a, NkB<BN, true>{.b = B, .ldb = p.ldb, .N = p.N, .K = p.K}, p.M, p.K, epi);
    };
    if constexpr (AMODE == A_PATCH)
        run(PatchA{p});
    else if constexpr (AMODE == A_KM)
        run(KmA{.a = A, .lda = p.lda, .M = p.M, .K = p.K});
    else
        run(RowsA<BM, true>{.a = A, .lda = p.lda, .M = p.M, .K = p.K});
}

// x[crop][0] = cls + pos[0], x[crop][1 + t] = emb[crop][t] + pos[1 + t]
__global__ __launch_bounds__(TPB) void maniqa_tokens_kernel(const float* __restrict__ emb, const float* __restrict__ pos, const float* __restrict__ cls, int T, int C,
                                                            long total, float* __restrict__ x) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long row = i / C;
    const int t = (int)(row % T);
    const long b = row / T;
    const float v = t == 0 ? cls[c] : emb[(b * (T - 1) + t - 1) * C + c];
    x[i] = v + pos[(long)t * C + c];
}

// out[b][c][r] = in[b][r][c] for r < R, c < C: rows of ld_in floats, a batch moves by in_stride / out_stride; 32 x 32 tiles through LDS
__global__ __launch_bounds__(TPB) void maniqa_transpose_kernel(const float* __restrict__ in, long ld_in, long in_stride, int R, int C, float* __restrict__ out,
                                                               long out_stride) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const float* src = in + (long)blockIdx.z * in_stride;
    float* dst = out + (long)blockIdx.z * out_stride;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < C) t[j][tx] = src[(long)(r0 + j) * ld_in + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < C && r0 + tx < R) dst[(long)(c0 + j) * R + r0 + tx] = t[tx][j];
}

// x0 = scale * y + x0 (a Swin layer's output enters its input), and a copy of the result into feat when given
__global__ __launch_bounds__(TPB) void maniqa_scale_add_kernel(const float* __restrict__ y, float* __restrict__ x0, float scale, long total, float* __restrict__ feat) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    float v = y[i] * scale;
    v = v + x0[i];
    x0[i] = v;
    if (feat) feat[i] = v;
}

// Window attention of one (crop, window, head) per wave. qkv: [crops * G * G][3 D] (q | k | v, heads of hd inside each), out: [crops * G * G][D].
__global__ __launch_bounds__(64) void maniqa_window_kernel(const float* __restrict__ qkv, const float* __restrict__ rpb, float* __restrict__ out, int G, int ws,
                                                           int heads, int hd, int shift, float scale, long total) {
    __shared__ float s_p[32][33];
    __shared__ int s_tok[32], s_lab[32];
    const long id = blockIdx.x;
    if (id >= total) return;
    const int lane = threadIdx.x, l31 = lane & 31, kh = lane >> 5;
    const int nw = G / ws, W = ws * ws, D = heads * hd;
    const int head = (int)(id % heads), win = (int)((id / heads) % (nw * nw));
    const long b = id / ((long)heads * nw * nw);
    const int wy = win / nw, wx = win - wy * nw;
    if (lane < 32) {
        int tok = -1, lab = 0;
        if (lane < W) {
            const int sy = wy * ws + lane / ws, sx = wx * ws + lane % ws;   // in the shifted grid: shifted[sy] = grid[(sy + shift) % G]
            tok = ((sy + shift) % G) * G + (sx + shift) % G;
            if (shift) lab = 3 * (sy < G - ws ? 0 : sy < G - shift ? 1 : 2) + (sx < G - ws ? 0 : sx < G - shift ? 1 : 2);
        }
        s_tok[lane] = tok;
        s_lab[lane] = lab;
    }
    __syncthreads();
    const int myt = s_tok[l31];
    const float* base = qkv + b * (long)G * G * 3 * D + head * hd;
    const float* qrow = base + (long)max(myt, 0) * 3 * D;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = 0; k < hd; k += 2) {
        float a = 0.f, bb = 0.f;
        if (myt >= 0) {
            a = qrow[k + kh] * scale;
            bb = qrow[D + k + kh];
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s_p[mfma_row(r, lane)][l31] = acc[r];
    __syncthreads();
    if (lane < 32) {   // row `lane`: + bias, + mask, softmax in key order
        const int i = lane;
        if (i < W) {
            const int iy = i / ws, ix = i % ws;
            float mx = -INFINITY;
            for (int j = 0; j < W; ++j) {
                const int idx = (iy - j / ws + ws - 1) * (2 * ws - 1) + ix - j % ws + ws - 1;
                float v = s_p[i][j] + rpb[(long)idx * heads + head];
                if (s_lab[i] != s_lab[j]) v = v + -100.0f;
                s_p[i][j] = v;
                mx = fmaxf(mx, v);
            }
            double sum = 0.0;
            for (int j = 0; j < W; ++j) sum += exp((double)s_p[i][j] - (double)mx);
            for (int j = 0; j < 32; ++j) s_p[i][j] = j < W ? (float)(exp((double)s_p[i][j] - (double)mx) / sum) : 0.f;
        } else {
            for (int j = 0; j < 32; ++j) s_p[i][j] = 0.f;
        }
    }
    __syncthreads();
    const int Wp = (W + 1) & ~1;
    for (int c0 = 0; c0 < hd; c0 += 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k = 0; k < Wp; k += 2) {
            const int kt = s_tok[k + kh];
            const float bv = (kt >= 0 && c0 + l31 < hd) ? base[(long)kt * 3 * D + 2 * D + c0 + l31] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_p[l31][k + kh], bv, acc, 0, 0, 0);
        }
        if (c0 + l31 < hd) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, lane);
                if (row < W) out[(b * G * G + s_tok[row]) * D + head * hd + c0 + l31] = acc[r];
            }
        }
    }
}

// one wave per patch token: h [rows][2 Eh] holds fc1 of the score head | fc1 of the weight head; s = relu(w2s . relu(h) + b), w = sigmoid(...) in fp64
__global__ __launch_bounds__(TPB) void maniqa_heads_kernel(const float* __restrict__ h, long rows, int Eh, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           double* __restrict__ sw) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;   // uniform over the wave
    const float* q = h + row * 2 * Eh;
    double s = 0.0, w = 0.0;
    for (int c = lane; c < Eh; c += 64) {
        s += (double)fmaxf(q[c], 0.f) * (double)w2[c];
        w += (double)fmaxf(q[Eh + c], 0.f) * (double)w2[Eh + c];
    }
    s = wave_sum_d(s) + (double)b2[0];
    w = wave_sum_d(w) + (double)b2[1];
    if (lane == 0) {
        sw[2 * row] = s > 0.0 ? s : 0.0;
        sw[2 * row + 1] = 1.0 / (1.0 + exp(-w));
    }
}

// one workgroup per image: score = sum(w s) / (sum(w) + 1e-8) over its `count` patches - thread t sums the patches t, t + 256, ... in order, the
// threads fold in a fixed tree
__global__ __launch_bounds__(TPB) void maniqa_pool_kernel(const double* __restrict__ sw, long count, int n, double* __restrict__ scores) {
    __shared__ double s_n[TPB], s_d[TPB];
    const int im = blockIdx.x, t = threadIdx.x;
    if (im >= n) return;
    const double* q = sw + 2 * (long)im * count;
    double num = 0.0, den = 0.0;
    for (long i = t; i < count; i += TPB) {
        num += q[2 * i + 1] * q[2 * i];
        den += q[2 * i + 1];
    }
    s_n[t] = num;
    s_d[t] = den;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (t < o) {
            s_n[t] += s_n[t + o];
            s_d[t] += s_d[t + o];
        }
        __syncthreads();
    }
    if (t == 0) scores[im] = s_n[0] / (s_d[0] + 1e-8);
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
GemmArgs gemm_args(const float* a, long lda, const float* b, long ldb, int M, int N, int K, const float* bias, const float* res, float* c, long ldc) {
    GemmArgs p{};
    p.a = a; p.lda = lda; p.b = b; p.ldb = ldb; p.Kb = K; p.M = M; p.N = N; p.K = K;
    p.bias = bias; p.res = res; p.alpha = 1.f; p.c = c; p.ldc = ldc; p.zdiv = 1;
    return p;
}
template <int AMODE, int BMODE>
void launch_gemm(const GemmArgs& p, int z, hipStream_t s) {
    hipLaunchKernelGGL((maniqa_gemm_kernel<AMODE, BMODE>), dim3((unsigned)((p.M + BM - 1) / BM), (unsigned)((p.N + BN - 1) / BN), (unsigned)z), dim3(TPB), 0, s, p);
}

}  // namespace

void ir_maniqa_input_table_host(float* tab) {
    for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
        volatile float x = (float)v / 255.0f;
        volatile float y = x - 0.5f;
        tab[v] = y / 0.5f;
    }
}

int ir_maniqa_crops_host(int h, int w, int crop, int crops, int* out_yx) {
    if (crop < 1 || crops < 1 || crops > IR_MANIQA_MAX_CROPS || std::min(h, w) <= crop || !out_yx) return -1;
    int lo = 1, hi = 1;
    while ((lo + 1) * (lo + 1) <= crops) ++lo;   // floor(sqrt(crops))
    while (hi * hi < crops) ++hi;                 // ceil(sqrt(crops))
    const int sh = (h - crop) / lo, sw = (w - crop) / lo;
    for (int k = 0; k < crops; ++k) {
        out_yx[2 * k] = (k / hi) * sh;
        out_yx[2 * k + 1] = (k % hi) * sw;
    }
    return 0;
}

int ir_maniqa_plan(const IrManiqaModel& m, int n, int crops, int per_pass, IrManiqaPlan* pl) {
    if (n < 1 || n > 4096 || crops < 1 || crops > IR_MANIQA_MAX_CROPS || per_pass < 1) return -1;
    const size_t total = (size_t)n * crops, cp = std::min<size_t>(std::min<size_t>(per_pass, total), 32768);
    const size_t G = m.crop / m.patch, N = G * G, T = N + 1, E = m.embed, C4 = 4 * E;
    if ((double)cp * T * std::max(m.vit_mlp, 3 * m.embed) > 2.0e9 * TPB || cp * T > (size_t)1 << 30 || cp * C4 * 3 * N > (size_t)1 << 40) return -1;
    pl->cp = (int)cp;
    pl->Tpad = (int)((T + BK - 1) / BK * BK);
    const size_t pair = T * pl->Tpad * sizeof(float);
    pl->zc = (int)std::min<size_t>(std::max<size_t>(SCORE_BYTES / pair, 1), std::min<size_t>(cp * m.vit_heads, 32768));
    size_t at = 0;
    pl->sw = at;
    at += up256(total * N * 2 * sizeof(double));
    pl->tap[0] = at;
    at += up256(cp * C4 * N * sizeof(float));
    pl->tap[1] = at;
    at += up256(cp * C4 * N * sizeof(float));
    size_t best = 0, tr = 0;
    auto take = [&](size_t floats) {
        const size_t o = at + tr;
        tr += up256(floats * sizeof(float));
        return o;
    };
    // the trunk
    pl->x = take(cp * T * E);
    pl->hn = take(cp * T * E);
    pl->qkv = take(cp * T * 3 * E);
    pl->o = take(cp * T * E);
    pl->f = take(cp * T * m.vit_mlp);
    pl->s = take((size_t)pl->zc * T * pl->Tpad);
    pl->emb = take(cp * N * E);
    best = std::max(best, tr);
    // a TAB, over the trunk's arrays: q | k | v of every crop and ONE crop's C x C matrix
    tr = 0;
    pl->tqkv = take(cp * C4 * 3 * N);
    pl->ts = take(C4 * C4);
    best = std::max(best, tr);
    // a Swin stage and the heads, likewise
    tr = 0;
    pl->y0 = take(cp * N * E);
    pl->y = take(cp * N * E);
    pl->yn = take(cp * N * E);
    pl->sqkv = take(cp * N * 3 * E);
    pl->so = take(cp * N * E);
    pl->sf = take(cp * N * std::max(m.dim_mlp, m.embed));
    best = std::max(best, tr);
    pl->total = at + best;
    return 0;
}

int ir_launch_maniqa(const IrManiqaModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, const int* origins, int crops, double* scores,
                     float* feat, void* ws, const IrManiqaPlan& pl, hipStream_t s) {
    char* base = static_cast<char*>(ws);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    double* SW = reinterpret_cast<double*>(base + pl.sw);
    const int G = m.crop / m.patch, N = G * G, T = N + 1, E = m.embed, Eh = E / 2, hd = E / m.vit_heads;
    const long total = (long)n * crops;
    float *X = at(pl.x), *HN = at(pl.hn), *QKV = at(pl.qkv), *O = at(pl.o), *F = at(pl.f), *S = at(pl.s), *EMB = at(pl.emb);
    float *TQKV = at(pl.tqkv), *TS = at(pl.ts);
    float *Y0 = at(pl.y0), *Y = at(pl.y), *YN = at(pl.yn), *SQKV = at(pl.sqkv), *SO = at(pl.so), *SF = at(pl.sf);

    for (long g0 = 0; g0 < total; g0 += pl.cp) {
        const int cc = (int)std::min<long>(pl.cp, total - g0);
        const long R = (long)cc * T;
        {   // the patch conv straight from the bytes, then the tokens
            GemmArgs p = gemm_args(nullptr, 0, m.patch_w, E, cc * N, E, 3 * m.patch * m.patch, m.patch_b, nullptr, EMB, E);
            p.img = img; p.pitch = pitch; p.img_stride = (long)rows * pitch; p.origins = origins; p.tab = m.tab;
            p.g0 = (int)g0; p.crops = crops; p.h = h; p.w = w; p.crop = m.crop; p.patch = m.patch; p.G = G;
            launch_gemm<A_PATCH, B_KN>(p, 1, s);
            hipLaunchKernelGGL(maniqa_tokens_kernel, dim3(blocks_of(R * E, TPB)), dim3(TPB), 0, s, EMB, m.pos, m.cls, T, E, R * E, X);
        }
        float* cur = at(pl.tap[0]);   // the map the next TAB reads
        float* oth = at(pl.tap[1]);
        const int pairs = cc * m.vit_heads;
        for (int l = 0, tap = 0; l < m.vit_layers; ++l) {
            const IrManiqaBlock& b = m.vit[l];
            launch_ln(X, R, E, b.ln1g, b.ln1b, 1e-6, HN, s);
            GemmArgs p = gemm_args(HN, E, b.qkvw, 3 * E, (int)R, 3 * E, E, b.qkvb, nullptr, QKV, 3 * E);
            launch_gemm<A_ROWS, B_KN>(p, 1, s);
            for (int z0 = 0; z0 < pairs; z0 += pl.zc) {
                const int z = std::min(pl.zc, pairs - z0);
                p = gemm_args(QKV, 3 * E, QKV + E, 3 * E, T, T, hd, nullptr, nullptr, S, pl.Tpad);   // (q k^T) * hd^-0.5
                p.alpha = 1.0f / sqrtf((float)hd);
                p.z0 = z0; p.zdiv = m.vit_heads;
                p.a_s0 = p.b_s0 = (long)T * 3 * E; p.a_s1 = p.b_s1 = hd; p.c_sl = (long)T * pl.Tpad;
                launch_gemm<A_ROWS, B_NK>(p, z, s);
                launch_softmax(S, (long)z * T, T, pl.Tpad, s);
                p = gemm_args(S, pl.Tpad, QKV + 2 * E, 3 * E, T, hd, pl.Tpad, nullptr, nullptr, O, E);   // p v; the padded columns of p are 0
                p.Kb = T;
                p.z0 = z0; p.zdiv = m.vit_heads;
                p.a_sl = (long)T * pl.Tpad; p.b_s0 = (long)T * 3 * E; p.b_s1 = hd; p.c_s0 = (long)T * E; p.c_s1 = hd;
                launch_gemm<A_ROWS, B_KN>(p, z, s);
            }
            p = gemm_args(O, E, b.pw, E, (int)R, E, E, b.pb, X, X, E);
            launch_gemm<A_ROWS, B_KN>(p, 1, s);
            launch_ln(X, R, E, b.ln2g, b.ln2b, 1e-6, HN, s);
            p = gemm_args(HN, E, b.f1w, m.vit_mlp, (int)R, m.vit_mlp, E, b.f1b, nullptr, F, m.vit_mlp);
            launch_gemm<A_ROWS, B_KN>(p, 1, s);
            launch_gelu(F, R * m.vit_mlp, s);
            p = gemm_args(F, m.vit_mlp, b.f2w, E, (int)R, E, m.vit_mlp, b.f2b, X, X, E);
            launch_gemm<A_ROWS, B_KN>(p, 1, s);
            if (tap < 4 && m.taps[tap] == l) {   // the patch tokens [N][E] of every crop -> rows tap * E .. of its map [4 E][N]
                hipLaunchKernelGGL(maniqa_transpose_kernel, dim3((E + 31) / 32, (N + 31) / 32, cc), dim3(TPB), 0, s, X + E, (long)E, (long)T * E, N, E,
                                   cur + (long)tap * E * N, (long)4 * E * N);
                ++tap;
            }
        }
        for (int st = 0; st < 2; ++st) {
            const int C = st == 0 ? 4 * E : E, D = st == 0 ? E : Eh, mlp = st == 0 ? m.dim_mlp : m.dim_mlp / 2, shd = D / m.swin_heads;
            for (int t = 0; t < 2; ++t) {   // TAB: cur [C][N] -> oth
                GemmArgs p = gemm_args(cur, N, m.tabw[st][t], 3 * N, C, 3 * N, N, m.tabb[st][t], nullptr, TQKV, 3 * N);
                p.a_s0 = (long)C * N; p.c_s0 = (long)C * 3 * N;
                launch_gemm<A_ROWS, B_KN>(p, cc, s);
                for (int j = 0; j < cc; ++j) {
                    const float* q = TQKV + (long)j * C * 3 * N;
                    p = gemm_args(q, 3 * N, q + N, 3 * N, C, C, N, nullptr, nullptr, TS, C);   // (q k^T) * N^-0.5
                    p.alpha = 1.0f / sqrtf((float)N);
                    launch_gemm<A_ROWS, B_NK>(p, 1, s);
                    launch_softmax(TS, (long)C, C, C, s);
                    p = gemm_args(TS, C, q + 2 * N, 3 * N, C, N, C, nullptr, cur + (long)j * C * N, oth + (long)j * C * N, C);
                    p.tstore = 1;   // element [c][n] at n * C + c, the residual from the same address of the input map
                    launch_gemm<A_ROWS, B_KN>(p, 1, s);
                }
                std::swap(cur, oth);
            }
            {   // the 1 x 1 conv: tokens [N][D] of the map [C][N], which is the A operand k-major as it lies
                GemmArgs p = gemm_args(cur, N, m.convw[st], D, N, D, C, m.convb[st], nullptr, Y0, D);
                p.a_s0 = (long)C * N; p.c_s0 = (long)N * D;
                launch_gemm<A_KM, B_KN>(p, cc, s);
            }
            const long RS = (long)cc * N;
            for (int l = 0; l < IR_MANIQA_SWIN_LAYERS; ++l) {
                for (int k = 0; k < m.swin_depth; ++k) {
                    const IrManiqaBlock& b = m.swin[st][l][k];
                    const float* in = k == 0 ? Y0 : Y;
                    launch_ln(in, RS, D, b.ln1g, b.ln1b, 1e-5, YN, s);
                    GemmArgs p = gemm_args(YN, D, b.qkvw, 3 * D, (int)RS, 3 * D, D, b.qkvb, nullptr, SQKV, 3 * D);
                    launch_gemm<A_ROWS, B_KN>(p, 1, s);
                    const long wtotal = (long)cc * (G / m.window) * (G / m.window) * m.swin_heads;
                    hipLaunchKernelGGL(maniqa_window_kernel, dim3((unsigned)wtotal), dim3(64), 0, s, SQKV, b.rpb, SO, G, m.window, m.swin_heads, shd,
                                       (k & 1) ? m.window / 2 : 0, 1.0f / sqrtf((float)shd), wtotal);
                    p = gemm_args(SO, D, b.pw, D, (int)RS, D, D, b.pb, in, Y, D);
                    launch_gemm<A_ROWS, B_KN>(p, 1, s);
                    launch_ln(Y, RS, D, b.ln2g, b.ln2b, 1e-5, YN, s);
                    p = gemm_args(YN, D, b.f1w, mlp, (int)RS, mlp, D, b.f1b, nullptr, SF, mlp);
                    launch_gemm<A_ROWS, B_KN>(p, 1, s);
                    launch_gelu(SF, RS * mlp, s);
                    p = gemm_args(SF, mlp, b.f2w, D, (int)RS, D, mlp, b.f2b, Y, Y, D);
                    launch_gemm<A_ROWS, B_KN>(p, 1, s);
                }
                float* f = (st == 1 && l + 1 == IR_MANIQA_SWIN_LAYERS && feat) ? feat + g0 * N * Eh : nullptr;
                hipLaunchKernelGGL(maniqa_scale_add_kernel, dim3(blocks_of(RS * D, TPB)), dim3(TPB), 0, s, Y, Y0, m.scale, RS * D, f);
            }
            if (st == 0)   // the tokens [N][E] back to a map [E][N] for the second pair of TABs
                hipLaunchKernelGGL(maniqa_transpose_kernel, dim3((E + 31) / 32, (N + 31) / 32, cc), dim3(TPB), 0, s, Y0, (long)E, (long)N * E, N, E, cur, (long)E * N);
        }
        {   // the heads: fc1 of both side by side, then one wave per patch token
            const long RS = (long)cc * N;
            GemmArgs p = gemm_args(Y0, Eh, m.head_w1, 2 * Eh, (int)RS, 2 * Eh, Eh, m.head_b1, nullptr, SQKV, 2 * Eh);
            launch_gemm<A_ROWS, B_KN>(p, 1, s);
            hipLaunchKernelGGL(maniqa_heads_kernel, dim3(blocks_of(RS, TPB / 64)), dim3(TPB), 0, s, SQKV, RS, Eh, m.head_w2, m.head_b2, SW + 2 * g0 * N);
        }
    }
    hipLaunchKernelGGL(maniqa_pool_kernel, dim3(n), dim3(TPB), 0, s, SW, (long)crops * N, n, scores);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
