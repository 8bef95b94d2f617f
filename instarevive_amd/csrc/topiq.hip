// TOPIQ-NR of uint8 HWC RGB device images (ir_topiq): the model of tools/evaluate_topiq.py - a ResNet-50 trunk at the image's own size, per
// feature level a gated local pooling, an adaptive pooling to the coarsest grid, a 1 x 1 reduction, an interpolated position table and one
// encoder layer, then the coarse-to-fine cross-attention, one more encoder layer and a small head - in exact fp32 with fp64 statistics.
//   Convolutions: implicit GEMMs on the exact-fp32 tile loop of exact_f32_tile.h (an output element depends neither on the tile it falls in nor
//   on the image's place in a batch), NHWC fp32 maps, weights repacked to [K padded to 32][cout] by ir_topiq_configure. The stem gathers from the
//   bytes through the 3 x 256 table (K = 147 padded to 160; padding is 0 in that domain); the stride-2 3 x 3 and 1 x 1 convs use the strided
//   operand. Epilogue: acc * scale[c] + shift[c] (the folded BatchNorm) or acc + bias[c], a residual add, a ReLU - separate roundings, the file
//   is built with -ffp-contract=off. Channel counts are multiples of 4, not of the tile: columns at or behind N read as zeros and are not stored.
//   Token GEMMs (splitconv, the gate's 1 x 1, dim_reduce, q | k | v, out, FFN) and Q K^T / P V: one GEMM kernel on the same loop, as musiq.hip
//   and maniqa.hip have it; q is scaled by hd^-0.5 in the epilogue of its projection, before Q K^T, as nn.MultiheadAttention does. The score
//   matrices of as many (image, head) pairs as fit SCORE_BYTES are live at a time.
//   Own kernels: the max pool; the 64 -> 1 gate conv fused with the sigmoid and gelu(x1) * w (one lane per pixel, one k-ordered fmaf chain);
//   the adaptive pool (fp64 bin sums in row, column order, rounded once); the position table (torch's bicubic in fp64, x first, then y, rounded
//   once) added to the tokens; LayerNorm, softmax and GELU of exact_rows.h; the level means; and everything from the token mean on in fp64, one
//   workgroup per image. No floating-point atomics: every sum is a sequential chain plus a fixed fold.
// Reads are clipped to the scored rectangle h x w; every store is guarded by the row count of its launch.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "exact_f32_tile.h"
#include "exact_rows.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int BN = 64;
constexpr int SMALL_GRID = 512;                   // below this many 128-row workgroups a conv takes the 64-row tile
constexpr size_t SCORE_BYTES = (size_t)1 << 26;   // the score matrices of one attention launch: as many (image, head) pairs as fit, at least one
constexpr int GH = IR_TOPIQ_GATE_HIDDEN;

// ---------------------------------------------------------------- convolutions
struct ConvArgs {
    const uint8_t* img;   // stem: the byte images
    long pitch, img_stride;
    const float* tab;     // [3][256]
    const float* in;      // else: an NHWC fp32 map [imgs][H][W][cin]
    int H, W, cin, Ho, Wo, ks, stride, pad;
    int M, K, Kpad, N;    // M = imgs * Ho * Wo, K = ks * ks * cin, N = cout
    const float* wgt;     // [Kpad][N]
    const float *scale, *shift;   // [N]; scale null: shift is the bias
    const float* res;     // [M][N] or null
    int relu;
    float* out;           // [M][N]
};

struct ConvEpi {
    const ConvArgs& p;
    int col;
    float sc, sh;
    IR_DEVINL bool column(int c) {
        if (c >= p.N) return false;
        col = c;
        sc = p.scale ? p.scale[c] : 1.f;
        sh = p.shift[c];
        return true;
    }
    IR_DEVINL void store(int m, float acc) const {
        float v = p.scale ? acc * sc : acc;
        v = v + sh;
        if (p.res) v = v + p.res[(long)m * p.N + col];
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[(long)m * p.N + col] = v;
    }
};

enum { CONV_STEM = 0, CONV_TAP = 1, CONV_ANY = 2 };   // TAP: cin is a multiple of 32, a k-tile never crosses a tap

template <int BM, int MODE>
__global__ __launch_bounds__(TPB, MODE == CONV_STEM ? 3 : BM == 64 ? 6 : 4) void topiq_conv_kernel(ConvArgs p) {
    const KnB<BN, true> b{.b = p.wgt, .ldb = p.N, .Kb = p.Kpad, .N = p.N};
    if constexpr (MODE == CONV_STEM) {
        __shared__ float s_tab[3 * 256];
        const ByteTableA<BM, false> a{.a = p.img, .a_pitch = p.pitch, .a_img = p.img_stride, .tab = p.tab, .s_tab = s_tab, .H = p.H, .W = p.W, .Ho = p.Ho, .Wo = p.Wo,
                                      .row_k = 3 * p.ks, .stride = p.stride, .pad = p.pad, .M = p.M, .K = p.K};
        tile_loop<BM, BN>(a, b, p.M, p.K, ConvEpi{p});
    } else {
        const NhwcA<BM, MODE == CONV_TAP> a{.in = p.in, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.cin, .kw = p.ks, .stride = p.stride, .ph = p.pad, .pw = p.pad,
                                            .Ho = p.Ho, .Wo = p.Wo, .M = p.M, .K = p.K};
        tile_loop<BM, BN>(a, b, p.M, p.K, ConvEpi{p});
    }
}

// ---------------------------------------------------------------- token GEMMs
enum { B_KN = 0, B_NK = 1 };
struct GemmArgs {
    const float* a;   // [M][lda]
    long lda;
    const float* b;   // B_KN: [K][ldb], B_NK: [N][ldb]
    long ldb;
    int Kb;           // B_KN: rows at or behind it read as zero
    int M, N, K;      // operands at or behind K read as zero; K a multiple of 4
    const float *bias, *res;   // [N] / [M][ldc], or null
    float alpha;      // columns below alpha_cols: (acc + bias) * alpha
    int alpha_cols;
    float* c;
    long ldc;
    // grid.z: pair z0 + blockIdx.z is (image, head) = (pair / zdiv, pair % zdiv); an operand moves by s0 per image, s1 per head, sl per blockIdx.z
    int z0, zdiv;
    long a_s0, a_s1, a_sl, b_s0, b_s1, c_s0, c_s1, c_sl;
};

struct GemmEpi {
    const GemmArgs& p;
    float* c;
    int col;
    float bs;
    IR_DEVINL bool column(int n) {
        if (n >= p.N) return false;
        col = n;
        bs = p.bias ? p.bias[n] : 0.f;
        return true;
    }
    IR_DEVINL void store(int m, float acc) const {
        const long at = (long)m * p.ldc + col;
        float v = acc;
        if (p.bias) v = v + bs;
        if (col < p.alpha_cols) v = v * p.alpha;
        if (p.res) v = v + p.res[at];
        c[at] = v;
    }
};

template <int BMODE>
__global__ __launch_bounds__(TPB, 4) void topiq_gemm_kernel(GemmArgs p) {
    constexpr int BM = 128;
    const int pair = p.z0 + (int)blockIdx.z, zi = pair / p.zdiv, zj = pair - zi * p.zdiv;
    const float* A = p.a + zi * p.a_s0 + zj * p.a_s1 + (long)blockIdx.z * p.a_sl;
    const float* B = p.b + zi * p.b_s0 + zj * p.b_s1;
    const GemmEpi epi{p, p.c + zi * p.c_s0 + zj * p.c_s1 + (long)blockIdx.z * p.c_sl};
    const RowsA<BM, true> a{.a = A, .lda = p.lda, .M = p.M, .K = p.K};
    if constexpr (BMODE == B_KN)
        tile_loop<BM, BN>(a, KnB<BN, true>{.b = B, .ldb = p.ldb, .Kb = p.Kb, .N = p.N}, p.M, p.K, epi);
    else
        tile_loop<BM, BN>(a, NkB<BN, true>{.b = B, .ldb = p.ldb, .N = p.N, .K = p.K}, p.M, p.K, epi);
}

// ---------------------------------------------------------------- own kernels
// MaxPool 3 x 3 / 2 / pad 1: the maximum over the taps inside the map
__global__ __launch_bounds__(TPB) void topiq_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int Ho, int Wo, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const long img = r / Ho;
    float m = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            m = fmaxf(m, in[((img * H + iy) * W + ix) * C + c]);
        }
    }
    out[i] = m;
}

IR_DEVINL float gelu_exact(float x) {
    const double v = (double)x;
    return (float)(0.5 * v * (1.0 + erf(v * 0.70710678118654752440)));
}

// The gate's last conv (3 x 3, 64 -> 1, pad 1), the sigmoid and x1 <- gelu(x1) * w for the TPB pixels of a workgroup. A lane owns a pixel: one
// fmaf chain from 0 over (ky, kx, c) - a tap outside the map is a run of fmaf(0, w, acc) = acc and is skipped - then + bias, the sigmoid in
// fp64. The product runs over the workgroup's TPB x C elements of x1 in order, in place.
__global__ __launch_bounds__(TPB) void topiq_gate_kernel(const float* __restrict__ h2, const float* __restrict__ w3, const float* __restrict__ b3, float* __restrict__ x1,
                                                         int H, int W, int C, long M) {
    __shared__ float s_w3[9 * GH];
    __shared__ float s_g[TPB];
    const int t = threadIdx.x;
    for (int i = t; i < 9 * GH; i += TPB) s_w3[i] = w3[i];
    __syncthreads();
    const long m0 = (long)blockIdx.x * TPB, m = m0 + t;
    float g = 0.f;
    if (m < M) {
        const int ox = (int)(m % W), oy = (int)((m / W) % H);
        const long img = m / ((long)H * W);
        float acc = 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                const float4* q = reinterpret_cast<const float4*>(h2 + ((img * H + iy) * W + ix) * GH);
                const float* wk = s_w3 + (ky * 3 + kx) * GH;
#pragma unroll 4
                for (int c4 = 0; c4 < GH / 4; ++c4) {
                    const float4 v = q[c4];
                    acc = fmaf(v.x, wk[4 * c4], acc);
                    acc = fmaf(v.y, wk[4 * c4 + 1], acc);
                    acc = fmaf(v.z, wk[4 * c4 + 2], acc);
                    acc = fmaf(v.w, wk[4 * c4 + 3], acc);
                }
            }
        }
        acc = acc + b3[0];
        g = (float)(1.0 / (1.0 + exp(-(double)acc)));
    }
    s_g[t] = g;
    __syncthreads();
    const long left = M - m0, cnt = (left < TPB ? left : (long)TPB) * C;
    float* base = x1 + m0 * C;
    for (long i = t; i < cnt; i += TPB) base[i] = gelu_exact(base[i]) * s_g[(int)(i / C)];
}

// adaptive_avg_pool2d to th x tw: bin i covers floor(i H / th) .. ceil((i + 1) H / th) - 1; the fp64 sum runs over the bin's rows, inside a row
// over its columns, is divided by the count and rounded once
__global__ __launch_bounds__(TPB) void topiq_adaptive_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int th, int tw, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ox = (int)(r % tw);
    r /= tw;
    const int oy = (int)(r % th);
    const long img = r / th;
    const int y0 = (int)(((long)oy * H) / th), y1 = (int)((((long)oy + 1) * H + th - 1) / th);
    const int x0 = (int)(((long)ox * W) / tw), x1 = (int)((((long)ox + 1) * W + tw - 1) / tw);
    double s = 0.0;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) s += (double)in[((img * H + y) * W + x) * C + c];
    out[i] = (float)(s / (double)((y1 - y0) * (x1 - x0)));
}

// torch's bicubic along one axis of IR_TOPIQ_EMB entries (align_corners=False, A = -0.75, clamped taps), in fp64 as the model writes it
IR_DEVINL void bicubic_axis(int i, int n_out, int (&tap)[4], double (&cf)[4]) {
    constexpr double A = -0.75;
    const double src = ((double)IR_TOPIQ_EMB / (double)n_out) * ((double)i + 0.5) - 0.5;
    const double f = floor(src), t = src - f;
    cf[0] = ((A * (t + 1.0) - 5.0 * A) * (t + 1.0) + 8.0 * A) * (t + 1.0) - 4.0 * A;
    cf[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    cf[2] = ((A + 2.0) * (1.0 - t) - (A + 3.0)) * (1.0 - t) * (1.0 - t) + 1.0;
    cf[3] = ((A * (2.0 - t) - 5.0 * A) * (2.0 - t) + 8.0 * A) * (2.0 - t) - 4.0 * A;
    const int f0 = (int)f;
#pragma unroll
    for (int k = 0; k < 4; ++k) tap[k] = min(max(f0 - 1 + k, 0), IR_TOPIQ_EMB - 1);
}

// x[img][y][x][c] += table(c, y, x) for the n images: channels below D / 2 interpolate h_emb (constant along x), the others w_emb (constant
// along y); x first, then y, each a four-term sum from the left, rounded once to fp32
__global__ __launch_bounds__(TPB) void topiq_pos_kernel(float* __restrict__ x, const float* __restrict__ h_emb, const float* __restrict__ w_emb, int H, int W, int D, int n,
                                                        long per_image) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= per_image) return;
    const int c = (int)(i % D), px = (int)((i / D) % W), py = (int)(i / ((long)D * W));
    int ty[4], tx[4];
    double cy[4], cx[4];
    bicubic_axis(py, H, ty, cy);
    bicubic_axis(px, W, tx, cx);
    const bool hpart = c < D / 2;
    const float* e = hpart ? h_emb + (long)c * IR_TOPIQ_EMB : w_emb + (long)(c - D / 2) * IR_TOPIQ_EMB;
    double rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = (double)e[hpart ? ty[k] : tx[j]] * cx[j];
        rows[k] = ((a[0] + a[1]) + a[2]) + a[3];
    }
    const float pos = (float)(((rows[0] * cy[0] + rows[1] * cy[1]) + rows[2] * cy[2]) + rows[3] * cy[3]);
    for (int im = 0; im < n; ++im) x[(long)im * per_image + i] = x[(long)im * per_image + i] + pos;
}

// out[img * out_stride + c] = (float)(sum over the T tokens / T). A workgroup takes 32 channels; token group g of 8 sums tokens g, g + 8, ... in
// order, the eight partial sums are added in order of g.
__global__ __launch_bounds__(TPB) void topiq_mean_kernel(const float* __restrict__ x, int T, int C, float* __restrict__ out, long out_stride) {
    __shared__ double s_part[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    double s = 0.0;
    if (c < C) {
        const float* q = x + (long)blockIdx.y * T * C + c;
        for (int t = g; t < T; t += 8) s += (double)q[(long)t * C];
    }
    s_part[g][cl] = s;
    __syncthreads();
    if (g == 0 && c < C) {
        double r = s_part[0][cl];
#pragma unroll
        for (int i = 1; i < 8; ++i) r += s_part[i][cl];
        out[(long)blockIdx.y * out_stride + c] = (float)(r / (double)T);
    }
}

// Everything from the token mean on, in fp64, one workgroup per image: feat = the mean over the T tokens (thread c sums its channel in token
// order), then LN, Linear, GELU, LN, Linear, GELU, Linear(D, 1). Every thread computes a LayerNorm's two sums itself, in channel order; an
// output of a Linear is one thread's chain in input order.
struct TailArgs {
    const float* x;   // [n][T][D]
    int T, D, n;
    const float *g0, *b0, *w1, *b1, *g3, *b3, *w4, *b4, *w6, *b6;
    double* scores;
    float* feat;      // [n][D] or null
};
constexpr int TAIL_MAX_D = 2048;

IR_DEVINL void tail_ln(const double* in, double* out, int D, const float* g, const float* b) {
    double mu = 0.0;
    for (int c = 0; c < D; ++c) mu += in[c];
    mu = mu / (double)D;
    double var = 0.0;
    for (int c = 0; c < D; ++c) {
        const double d = in[c] - mu;
        var += d * d;
    }
    const double rstd = 1.0 / sqrt(var / (double)D + 1e-5);
    for (int c = threadIdx.x; c < D; c += TPB) out[c] = (in[c] - mu) * rstd * (double)g[c] + (double)b[c];
}
IR_DEVINL void tail_linear_gelu(const double* in, double* out, int D, const float* w, const float* b) {
    for (int j = threadIdx.x; j < D; j += TPB) {
        const float* wj = w + (long)j * D;
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += (double)wj[c] * in[c];
        s = s + (double)b[j];
        out[j] = 0.5 * s * (1.0 + erf(s * 0.70710678118654752440));
    }
}

__global__ __launch_bounds__(TPB) void topiq_tail_kernel(TailArgs p) {
    __shared__ double s_a[TAIL_MAX_D], s_b[TAIL_MAX_D];
    const int img = blockIdx.x, t = threadIdx.x;
    if (img >= p.n) return;
    const int D = p.D;
    const float* x = p.x + (long)img * p.T * D;
    for (int c = t; c < D; c += TPB) {
        double s = 0.0;
        for (int k = 0; k < p.T; ++k) s += (double)x[(long)k * D + c];
        s = s / (double)p.T;
        s_a[c] = s;
        if (p.feat) p.feat[(long)img * D + c] = (float)s;
    }
    __syncthreads();
    tail_ln(s_a, s_b, D, p.g0, p.b0);
    __syncthreads();
    tail_linear_gelu(s_b, s_a, D, p.w1, p.b1);
    __syncthreads();
    tail_ln(s_a, s_b, D, p.g3, p.b3);
    __syncthreads();
    tail_linear_gelu(s_b, s_a, D, p.w4, p.b4);
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += (double)p.w6[c] * s_a[c];
        p.scores[img] = s + (double)p.b6[0];
    }
}

// ---------------------------------------------------------------- host
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
int down2(int s) { return (s - 1) / 2 + 1; }
int pad32i(int x) { return (x + 31) & ~31; }

void launch_conv(const IrTopiqConv& cv, const float* in, const float* res, int relu, float* out, int imgs, int H, int W, int Ho, int Wo, hipStream_t s) {
    ConvArgs p{};
    p.in = in; p.H = H; p.W = W; p.cin = cv.cin; p.Ho = Ho; p.Wo = Wo; p.ks = cv.ks; p.stride = cv.stride; p.pad = cv.ks / 2;
    p.M = imgs * Ho * Wo; p.K = cv.ks * cv.ks * cv.cin; p.Kpad = pad32i(p.K); p.N = cv.cout;
    p.wgt = cv.w; p.scale = cv.scale; p.shift = cv.shift; p.res = res; p.relu = relu; p.out = out;
    const unsigned gn = (unsigned)((p.N + BN - 1) / BN), gm = (unsigned)((p.M + 127) / 128), gs = (unsigned)((p.M + 63) / 64);
    const bool tap = cv.cin % BK == 0, small = (long)gm * gn < SMALL_GRID;
    // the tile does not change a single output (a k-ordered chain each): it is chosen for the grid alone
    if (tap && small) hipLaunchKernelGGL((topiq_conv_kernel<64, CONV_TAP>), dim3(gs, gn), dim3(TPB), 0, s, p);
    else if (tap) hipLaunchKernelGGL((topiq_conv_kernel<128, CONV_TAP>), dim3(gm, gn), dim3(TPB), 0, s, p);
    else if (small) hipLaunchKernelGGL((topiq_conv_kernel<64, CONV_ANY>), dim3(gs, gn), dim3(TPB), 0, s, p);
    else hipLaunchKernelGGL((topiq_conv_kernel<128, CONV_ANY>), dim3(gm, gn), dim3(TPB), 0, s, p);
}

GemmArgs gemm_args(const float* a, long lda, const float* b, long ldb, int M, int N, int K, const float* bias, const float* res, float* c, long ldc) {
    GemmArgs p{};
    p.a = a; p.lda = lda; p.b = b; p.ldb = ldb; p.Kb = K; p.M = M; p.N = N; p.K = K;
    p.bias = bias; p.res = res; p.alpha = 1.f; p.alpha_cols = 0; p.c = c; p.ldc = ldc; p.zdiv = 1;
    return p;
}
template <int BMODE>
void launch_gemm(const GemmArgs& p, int z, hipStream_t s) {
    hipLaunchKernelGGL((topiq_gemm_kernel<BMODE>), dim3((unsigned)((p.M + 127) / 128), (unsigned)((p.N + BN - 1) / BN), (unsigned)z), dim3(TPB), 0, s, p);
}
// c[M][N] = a[M][K] w[K][N] + bias (+ res)
void linear(const float* a, const float* w, long ldw, const float* bias, const float* res, float* c, int M, int N, int K, hipStream_t s) {
    launch_gemm<B_KN>(gemm_args(a, K, w, ldw, M, N, K, bias, res, c, N), 1, s);
}

int score_pairs(int pairs, int Tq, int Tk) {
    const size_t per = (size_t)Tq * pad32i(Tk) * sizeof(float);
    return (int)std::min<size_t>(std::max<size_t>(SCORE_BYTES / per, 1), std::min<size_t>(pairs, 32768));
}

struct Run {
    const IrTopiqModel& m;
    const IrTopiqPlan& pl;
    int n;
    float *HN, *HM, *QKV, *O, *F, *S;
    hipStream_t s;

    // O[n][Tq][D] = softmax(Q K^T) V per (image, head); Q is scaled already
    void attention(const float* Q, long ldq, const float* K, long ldk, const float* V, long ldv, int Tq, int Tk) const {
        const int D = m.dim, hd = D / m.heads, pairs = n * m.heads, Tkpad = pad32i(Tk), zc = score_pairs(pairs, Tq, Tk);
        for (int z0 = 0; z0 < pairs; z0 += zc) {
            const int z = std::min(zc, pairs - z0);
            GemmArgs p = gemm_args(Q, ldq, K, ldk, Tq, Tk, hd, nullptr, nullptr, S, Tkpad);
            p.z0 = z0; p.zdiv = m.heads;
            p.a_s0 = (long)Tq * ldq; p.a_s1 = hd; p.b_s0 = (long)Tk * ldk; p.b_s1 = hd; p.c_sl = (long)Tq * Tkpad;
            launch_gemm<B_NK>(p, z, s);
            launch_softmax(S, (long)z * Tq, Tk, Tkpad, s);
            p = gemm_args(S, Tkpad, V, ldv, Tq, hd, Tkpad, nullptr, nullptr, O, D);   // the padded columns of the probabilities are 0
            p.Kb = Tk;
            p.z0 = z0; p.zdiv = m.heads;
            p.a_sl = (long)Tq * Tkpad; p.b_s0 = (long)Tk * ldv; p.b_s1 = hd; p.c_s0 = (long)Tq * D; p.c_s1 = hd;
            launch_gemm<B_KN>(p, z, s);
        }
    }
    void ffn(float* X, int R, const IrTopiqAttn& a, const float* g, const float* b) const {
        const int D = m.dim;
        launch_ln(X, R, D, g, b, 1e-5, HN, s);
        linear(HN, a.f1w, m.ffn, a.f1b, nullptr, F, R, m.ffn, D, s);
        launch_gelu(F, (long)R * m.ffn, s);
        linear(F, a.f2w, D, a.f2b, X, X, R, D, m.ffn, s);
    }
    // the pre-norm encoder layer, in place over X [n][T][D]
    void encoder(float* X, int T, const IrTopiqAttn& a) const {
        const int D = m.dim, R = n * T;
        launch_ln(X, R, D, a.n1g, a.n1b, 1e-5, HN, s);
        GemmArgs p = gemm_args(HN, D, a.inw, 3 * D, R, 3 * D, D, a.inb, nullptr, QKV, 3 * D);
        p.alpha = 1.0f / sqrtf((float)(D / m.heads)); p.alpha_cols = D;
        launch_gemm<B_KN>(p, 1, s);
        attention(QKV, 3 * D, QKV + D, 3 * D, QKV + 2 * D, 3 * D, T, T);
        linear(O, a.ow, D, a.ob, X, X, R, D, D, s);
        ffn(X, R, a, a.n2g, a.n2b);
    }
    // the coarse-to-fine layer: Q [n][Tq][D] in place, MEM [n][Tk][D]
    void decoder(float* Q, int Tq, const float* MEM, int Tk, const IrTopiqAttn& a) const {
        const int D = m.dim, Rq = n * Tq, Rk = n * Tk;
        launch_ln(MEM, Rk, D, a.n2g, a.n2b, 1e-5, HM, s);
        launch_ln(Q, Rq, D, a.n1g, a.n1b, 1e-5, HN, s);
        float *q = QKV, *kv = QKV + (size_t)Rq * D;
        GemmArgs p = gemm_args(HN, D, a.inw, 3 * D, Rq, D, D, a.inb, nullptr, q, D);
        p.alpha = 1.0f / sqrtf((float)(D / m.heads)); p.alpha_cols = D;
        launch_gemm<B_KN>(p, 1, s);
        launch_gemm<B_KN>(gemm_args(HM, D, a.inw + D, 3 * D, Rk, 2 * D, D, a.inb + D, nullptr, kv, 2 * D), 1, s);
        attention(q, D, kv, 2 * D, kv + D, 2 * D, Tq, Tk);
        linear(O, a.ow, D, a.ob, Q, Q, Rq, D, D, s);
        ffn(Q, Rq, a, a.n3g, a.n3b);
    }
};

}  // namespace

void ir_topiq_input_table_host(float* tab) {
    static const float mean[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
            volatile float x = (float)v / 255.0f;
            volatile float y = x - mean[ch];
            tab[256 * ch + v] = y / std3[ch];
        }
}

int ir_topiq_plan(const IrTopiqModel& m, int n, int h, int w, IrTopiqPlan* pl) {
    if (n < 1 || n > 65535 || h < IR_TOPIQ_MIN_EDGE || w < IR_TOPIQ_MIN_EDGE) return -1;
    const size_t D = m.dim;
    int H = down2(h), W = down2(w);
    if ((double)n * H * W > 2.0e9) return -1;   // M is an int
    size_t fl[5] = {0, 0, 0, 0, 0};   // floats per image of the five trunk slots
    pl->H[0] = H; pl->W[0] = W;
    fl[0] = (size_t)H * W * m.width;
    H = down2(H); W = down2(W);
    fl[1] = (size_t)H * W * m.width;
    int cur = 1, bi = 0;
    for (int l = 0; l < 4; ++l) {
        for (int i = 0; i < m.depths[l]; ++i, ++bi) {
            const IrTopiqBlock& b = m.blocks[bi];
            const int Ho = b.c2.stride == 2 ? down2(H) : H, Wo = b.c2.stride == 2 ? down2(W) : W;
            fl[2] = std::max(fl[2], (size_t)H * W * b.c1.cout);
            fl[3] = std::max(fl[3], (size_t)Ho * Wo * b.c2.cout);
            if (b.has_down) fl[4] = std::max(fl[4], (size_t)Ho * Wo * b.c3.cout);
            fl[1 - cur] = std::max(fl[1 - cur], (size_t)Ho * Wo * b.c3.cout);
            cur = 1 - cur;
            H = Ho; W = Wo;
        }
        pl->H[l + 1] = H; pl->W[l + 1] = W;
    }
    size_t at = 0;
    for (int k = 0; k < 5; ++k) {
        pl->slot[k] = at;
        at += up256((size_t)n * fl[k] * sizeof(float));
    }
    const int th = pl->H[4], tw = pl->W[4];
    size_t ga = 0, gh = 0, pooled = 0, Tmax = 0, sc = 0;
    for (int i = 0; i < 5; ++i) {
        const size_t C = (size_t)m.width << (i == 0 ? 0 : i + 1), px = (size_t)pl->H[i] * pl->W[i];
        const bool pool = pl->H[i] > th && pl->W[i] > tw;
        pl->TH[i] = pool ? th : pl->H[i];
        pl->TW[i] = pool ? tw : pl->W[i];
        const size_t T = (size_t)pl->TH[i] * pl->TW[i];
        ga = std::max(ga, px * C);
        gh = std::max(gh, px * GH);
        if (pool) pooled = std::max(pooled, T * C);
        Tmax = std::max(Tmax, T);
    }
    const int T4 = th * tw, pairs = n * m.heads;
    for (int i = 0; i < 5; ++i) {
        const int T = pl->TH[i] * pl->TW[i];
        sc = std::max(sc, (size_t)score_pairs(pairs, T, T) * T * pad32i(T));
        if (i < 4) sc = std::max(sc, (size_t)score_pairs(pairs, T4, T) * T4 * pad32i(T));
    }
    auto take = [&](size_t floats) {
        const size_t o = at;
        at += up256(floats * sizeof(float));
        return o;
    };
    pl->ga = take(n * ga);
    pl->gh1 = take(n * gh);
    pl->gh2 = take(n * gh);
    pl->pooled = take(n * pooled);
    for (int i = 0; i < 5; ++i) pl->tok[i] = take((size_t)n * pl->TH[i] * pl->TW[i] * D);
    pl->hn = take(n * Tmax * D);
    pl->hm = take(n * Tmax * D);
    pl->qkv = take(n * Tmax * 3 * D);
    pl->o = take(n * Tmax * D);
    pl->f = take(n * Tmax * m.ffn);
    pl->s = take(sc);
    pl->total = at;
    return 0;
}

int ir_launch_topiq(const IrTopiqModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, float* level_means, void* ws,
                    hipStream_t s) {
    IrTopiqPlan pl;
    if (ir_topiq_plan(m, n, h, w, &pl)) return -1;
    char* base = static_cast<char*>(ws);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float* S[5];
    for (int k = 0; k < 5; ++k) S[k] = at(pl.slot[k]);
    float *GA = at(pl.ga), *GH1 = at(pl.gh1), *GH2 = at(pl.gh2), *PL = at(pl.pooled);
    float* TOK[5];
    for (int k = 0; k < 5; ++k) TOK[k] = at(pl.tok[k]);
    const Run run{m, pl, n, at(pl.hn), at(pl.hm), at(pl.qkv), at(pl.o), at(pl.f), at(pl.s), s};
    const int D = m.dim;

    // a level's head: gate, adaptive pool, dim_reduce, position table, encoder layer, token mean
    auto level = [&](int i, const float* f) {
        const IrTopiqGate& g = m.gate[i];
        const int H = pl.H[i], W = pl.W[i], C = m.width << (i == 0 ? 0 : i + 1), M = n * H * W;
        linear(f, g.sw + C, 2 * C, g.sb + C, nullptr, GA, M, C, C, s);                     // x2
        linear(GA, g.w1, GH, g.b1, nullptr, GH1, M, GH, C, s);
        launch_gelu(GH1, (long)M * GH, s);
        launch_conv(g.c2, GH1, nullptr, 0, GH2, n, H, W, H, W, s);
        launch_gelu(GH2, (long)M * GH, s);
        linear(f, g.sw, 2 * C, g.sb, nullptr, GA, M, C, C, s);                             // x1, over x2
        hipLaunchKernelGGL(topiq_gate_kernel, dim3(blocks_of(M, TPB)), dim3(TPB), 0, s, GH2, g.w3, g.b3, GA, H, W, C, (long)M);
        const int TH = pl.TH[i], TW = pl.TW[i], T = TH * TW, R = n * T;
        const float* src = GA;
        if (TH != H || TW != W) {
            const long total = (long)R * C;
            hipLaunchKernelGGL(topiq_adaptive_pool_kernel, dim3(blocks_of(total, TPB)), dim3(TPB), 0, s, GA, PL, H, W, C, TH, TW, total);
            src = PL;
        }
        linear(src, g.rw, D, g.rb, nullptr, TOK[i], R, D, C, s);
        launch_gelu(TOK[i], (long)R * D, s);
        const long per = (long)T * D;
        hipLaunchKernelGGL(topiq_pos_kernel, dim3(blocks_of(per, TPB)), dim3(TPB), 0, s, TOK[i], m.h_emb, m.w_emb, TH, TW, D, n, per);
        run.encoder(TOK[i], T, m.sa[i]);
        if (level_means)
            hipLaunchKernelGGL(topiq_mean_kernel, dim3((unsigned)((D + 31) / 32), n), dim3(TPB), 0, s, TOK[i], T, D, level_means + (long)i * D, (long)5 * D);
    };

    int H = pl.H[0], W = pl.W[0];
    {   // the stem from the bytes -> S0 (feature 0), max pool -> S1
        const IrTopiqConv& cv = m.stem;
        ConvArgs p{};
        p.img = img; p.pitch = pitch; p.img_stride = (long)rows * pitch; p.tab = m.tab;
        p.H = h; p.W = w; p.cin = 3; p.Ho = H; p.Wo = W; p.ks = 7; p.stride = 2; p.pad = 3;
        p.M = n * H * W; p.K = 147; p.Kpad = pad32i(147); p.N = cv.cout;
        p.wgt = cv.w; p.scale = cv.scale; p.shift = cv.shift; p.res = nullptr; p.relu = 1; p.out = S[0];
        hipLaunchKernelGGL((topiq_conv_kernel<128, CONV_STEM>), dim3((unsigned)((p.M + 127) / 128), (unsigned)((p.N + BN - 1) / BN)), dim3(TPB), 0, s, p);
        level(0, S[0]);
        const int Ho = down2(H), Wo = down2(W);
        const long total = (long)n * Ho * Wo * m.width;
        hipLaunchKernelGGL(topiq_maxpool_kernel, dim3(blocks_of(total, TPB)), dim3(TPB), 0, s, S[0], S[1], H, W, m.width, Ho, Wo, total);
        H = Ho; W = Wo;
    }
    int cur = 1, bi = 0;
    for (int l = 0; l < 4; ++l) {
        for (int i = 0; i < m.depths[l]; ++i, ++bi) {
            const IrTopiqBlock& b = m.blocks[bi];
            const int Ho = b.c2.stride == 2 ? down2(H) : H, Wo = b.c2.stride == 2 ? down2(W) : W;
            const float* x = S[cur];
            const float* idn = x;
            if (b.has_down) {
                launch_conv(b.down, x, nullptr, 0, S[4], n, H, W, Ho, Wo, s);
                idn = S[4];
            }
            launch_conv(b.c1, x, nullptr, 1, S[2], n, H, W, H, W, s);
            launch_conv(b.c2, S[2], nullptr, 1, S[3], n, H, W, Ho, Wo, s);
            launch_conv(b.c3, S[3], idn, 1, S[1 - cur], n, Ho, Wo, Ho, Wo, s);
            cur = 1 - cur;
            H = Ho; W = Wo;
        }
        level(l + 1, S[cur]);
    }

    const int T4 = pl.TH[4] * pl.TW[4];
    float* Q = TOK[4];   // level 4's mean is taken; its tokens become the query
    for (int k = 0; k < 4; ++k) run.decoder(Q, T4, TOK[3 - k], pl.TH[3 - k] * pl.TW[3 - k], m.ca[k]);
    run.encoder(Q, T4, m.pool);
    TailArgs t{Q, T4, D, n, m.sc[0], m.sc[1], m.sc[2], m.sc[3], m.sc[4], m.sc[5], m.sc[6], m.sc[7], m.sc[8], m.sc[9], scores, feat};
    hipLaunchKernelGGL(topiq_tail_kernel, dim3(n), dim3(TPB), 0, s, t);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
