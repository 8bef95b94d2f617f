// MUSIQ of uint8 HWC RGB device images (ir_musiq): the model of tools/evaluate_musiq.py - the image at three scales, 32 x 32 patches with 'SAME'
// padding, a small ResNet stem per patch, the hashed spatial and the scale embedding, 14 pre-LN transformer blocks over all T tokens of the image,
// the final LayerNorm of the class token and a linear head - in exact fp32 with fp64 statistics.
//   Contractions: ONE GEMM kernel on the exact-fp32 tile loop of exact_f32_tile.h (an output element depends neither on the tile it falls in, nor
//   on T, nor on its place in a batch), 128 x 64 tiles. The A operand is row-major rows (the 1 x 1 convs on NHWC maps, the embedding, the linears, Q and the probabilities), the implicit im2col of
//   a 3 x 3 'SAME' conv over each patch's 8 x 8 map, or that of the 7 x 7 stride-2 stem conv over the patch's 32 x 32 x 3 input (K = 147, zero
//   behind it); the B operand is [K][N] (the repacked weights, V) or [N][K] (K of Q K^T). Rows of B at or behind Kb read as zero, as do the
//   padded columns of the probabilities: the PV product's K = T is padded with exact zeros. Epilogue: acc * alpha + bias[col] + residual, separate
//   roundings (the file is built with -ffp-contract=off). Attention runs zc (image, head) pairs per launch in grid.z: the score matrix is
//   zc * T * Tpad floats.
//   The patch kernel makes every patch's input: the byte through the 256-entry table ((v / 255 - 0.5) * 2 in fp32) at the image's own size, or
//   torch's bicubic (A = -0.75, align_corners = False, taps clamped, no antialias) of the table values for a resized scale - coordinates, weights and
//   the 16-tap sum in fp64, rounded once; 0 outside the scale's image ('SAME' padding in that domain). Reads are clipped to the scored rectangle.
//   GroupNorm (per patch) and the head: fp64 sums, each a per-lane sequential chain followed by a fixed butterfly; LayerNorm, the softmax rows
//   and the exact GELU are the kernels of exact_rows.h. An image gives the same bits on every call and at every place in a batch.
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
constexpr int PATCH = 32, PIN = PATCH * PATCH * 3;   // a patch's input values
constexpr int STEM_K = 147, STEM_O = 16, POOL_O = 8, STEM_C = 64, OUT_C = 256;   // 7 * 7 * 3; 32 -> 16 -> 8; channel counts of the stem
// The score matrices of one attention launch: as many (image, head) pairs as fit SCORE_BYTES, but the heads of one image together while they fit
// SCORE_MAX - at 2048 x 2048 the six matrices of 73 MB lie over the patch slots, which are far larger, and P V fills the device only with all of
// its heads in one grid. One pair is always taken whole.
constexpr size_t SCORE_BYTES = (size_t)1 << 23, SCORE_MAX = (size_t)1 << 30;

enum { A_ROWS = 0, A_CONV3 = 1, A_STEM = 2 };
enum { B_KN = 0, B_NK = 1 };

struct GemmArgs {
    const float* a;   // A_ROWS: [M][lda]; A_CONV3: NHWC maps [M / (H W)][H][W][cin]; A_STEM: [M / 256][32][32][3]
    long lda;
    int H, W, cin;
    const float* b;   // B_KN: [K][ldb], B_NK: [N][ldb]
    long ldb;
    int Kb;           // B_KN: rows at or behind it read as zero
    int M, N, K;      // K: a multiple of BK, except for A_STEM
    const float *bias, *res;   // [N] / [M][ldc], or null
    float alpha;
    float* c;
    long ldc;
    // grid.z: pair z0 + blockIdx.z is (image, head) = (pair / zdiv, pair % zdiv); an operand moves by s0 per image, s1 per head, sl per blockIdx.z
    int z0, zdiv;
    long a_s0, a_s1, a_sl, b_s0, b_s1, b_sl, c_s0, c_s1, c_sl;
};

// A_STEM: the implicit im2col of the 7 x 7 stride-2 'SAME' stem conv over fp32 patches [M / 256][32][32][3], K = 147 in (ky, kx, c) order
struct StemA {
    static constexpr int AR = BM * BK / TPB;
    const float* a;
    int M;
    long ro[AR];
    int riy[AR], rix[AR];
    float ga[AR];

    IR_DEVINL void rows(int m0) {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + ((int)threadIdx.x >> 5) + 8 * i;
            if (m < M) {
                const int pt = m / (STEM_O * STEM_O), r = m - pt * (STEM_O * STEM_O), oy = r / STEM_O, ox = r - oy * STEM_O;
                riy[i] = oy * 2 - 2;   // 'SAME' at stride 2: 2 in front, 3 behind
                rix[i] = ox * 2 - 2;
                ro[i] = (long)pt * PIN;
            } else {
                riy[i] = -(1 << 20);   // every tap out of bounds
                rix[i] = 0;
                ro[i] = 0;
            }
        }
    }
    IR_DEVINL void load(int k0) {
        const int k = k0 + ((int)threadIdx.x & 31);
        const int ky = k / 21, r = k - ky * 21, kx = r / 3, ch = r - kx * 3;   // 21 = 7 taps x 3 channels of one row
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int iy = riy[i] + ky, ix = rix[i] + kx;
            float v = 0.f;
            if (k < STEM_K && iy >= 0 && iy < PATCH && ix >= 0 && ix < PATCH) v = a[ro[i] + (iy * PATCH + ix) * 3 + ch];
            ga[i] = v;
        }
    }
    template <int LDA>
    IR_DEVINL void store(float (&s_a)[BK][LDA]) const { store_a_k1(s_a, ga); }
};

// acc * alpha + bias[col] + residual, separate roundings
struct AlphaBiasRes {
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
        float v = acc * p.alpha;   // 1 or a power of two: exact
        v = v + bs;
        if (p.res) v = v + p.res[(long)m * p.ldc + col];
        c[(long)m * p.ldc + col] = v;
    }
};

template <int AMODE, int BMODE>
__global__ __launch_bounds__(TPB, AMODE == A_STEM ? 3 : 4) void musiq_gemm_kernel(GemmArgs p) {
    const int pair = p.z0 + (int)blockIdx.z, zi = pair / p.zdiv, zj = pair - zi * p.zdiv;
    const float* A = p.a + zi * p.a_s0 + zj * p.a_s1 + (long)blockIdx.z * p.a_sl;
    const float* B = p.b + zi * p.b_s0 + zj * p.b_s1 + (long)blockIdx.z * p.b_sl;
    const AlphaBiasRes epi{p, p.c + zi * p.c_s0 + zj * p.c_s1 + (long)blockIdx.z * p.c_sl};
    const auto run = [&](auto a) {
        if constexpr (BMODE == B_KN)
            tile_loop<BM, BN>(a, KnB<BN, true>{.b = B, .ldb = p.ldb, .Kb = p.Kb, .N = p.N}, p.M, p.K, epi);
        else
            tile_loop<BM, BN>(a, NkB<BN, false>{.b = B, .ldb = p.ldb, .N = p.N, .K = p.K}, p.M, p.K, epi);
    };
    if constexpr (AMODE == A_STEM)
        run(StemA{.a = A, .M = p.M});
    else if constexpr (AMODE == A_CONV3)   // cin is a multiple of BK: a k-tile never crosses a tap
        run(NhwcA<BM, true>{.in = A, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.cin, .kw = 3, .stride = 1, .ph = 1, .pw = 1, .Ho = p.H, .Wo = p.W, .M = p.M, .K = p.K});
    else
        run(RowsA<BM, false>{.a = A, .lda = p.lda, .M = p.M, .K = p.K});
}

struct PatchArgs {
    const uint8_t* img;
    long pitch, img_stride;
    int h, w;
    const float* tab;   // [256]
    IrMusiqLayout lay;
    long total;         // n * patches * 32 * 32
    float* out;         // [n * patches][32][32][3]
};

// torch's cubic convolution coefficients for the taps -1 .. 2 at the fraction t, A = -0.75
IR_DEVINL void cubic_coefficients(double t, double* c) {
    const double A = -0.75;
    double x = t + 1.0;
    c[0] = ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A;
    x = t;
    c[1] = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
    x = 1.0 - t;
    c[2] = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
    x = 2.0 - t;
    c[3] = ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A;
}

// one thread per pixel of a patch
__global__ __launch_bounds__(TPB) void musiq_patch_kernel(PatchArgs p) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= p.total) return;
    const int px = (int)(i % PATCH), py = (int)((i / PATCH) % PATCH);
    const long pg = i / (PATCH * PATCH);
    const int im = (int)(pg / p.lay.patches), pp = (int)(pg - (long)im * p.lay.patches);
    int s = 0;
    while (s + 1 < p.lay.n_scales && pp >= p.lay.s[s + 1].first) ++s;
    const IrMusiqScale& g = p.lay.s[s];
    const int q = pp - g.first, gi = q / g.count_w, gj = q - gi * g.count_w;
    const int Y = gi * PATCH + py - g.pad_top, X = gj * PATCH + px - g.pad_left;
    float* o = p.out + i * 3;
    if (Y < 0 || Y >= g.rh || X < 0 || X >= g.rw) {
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const uint8_t* src = p.img + (long)im * p.img_stride;
    if (!g.resized) {
        const uint8_t* t = src + (long)Y * p.pitch + 3L * X;
        o[0] = p.tab[t[0]];
        o[1] = p.tab[t[1]];
        o[2] = p.tab[t[2]];
        return;
    }
    const double ry = ((double)p.h / (double)g.rh) * ((double)Y + 0.5) - 0.5, rx = ((double)p.w / (double)g.rw) * ((double)X + 0.5) - 0.5;
    const double fy = floor(ry), fx = floor(rx);
    double cy[4], cx[4];
    cubic_coefficients(ry - fy, cy);
    cubic_coefficients(rx - fx, cx);
    const int iy = (int)fy, ix = (int)fx;
    long xo[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) xo[b] = 3L * min(max(ix - 1 + b, 0), p.w - 1);
    double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint8_t* row = src + (long)min(max(iy - 1 + a, 0), p.h - 1) * p.pitch;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double r = (double)p.tab[row[xo[0] + ch]] * cx[0] + (double)p.tab[row[xo[1] + ch]] * cx[1] + (double)p.tab[row[xo[2] + ch]] * cx[2] +
                             (double)p.tab[row[xo[3] + ch]] * cx[3];
            sum[ch] = a == 0 ? r * cy[0] : sum[ch] + r * cy[a];
        }
    }
    o[0] = (float)sum[0];
    o[1] = (float)sum[1];
    o[2] = (float)sum[2];
}

// GroupNorm(32 groups) of the NHWC map [HW][C] of patch blockIdx.x, then + res, then ReLU. A wave takes groups wave, wave + 4, ...: lane l sums
// the group's elements l, l + 64, ... in order (element e = pixel e / cpg, channel e % cpg of the group), the lanes fold in a fixed butterfly.
// In place is allowed: a wave writes a group only after it has read all of it.
__global__ __launch_bounds__(TPB) void musiq_gn_kernel(const float* x, const float* res, float* out, int HW, int C, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, double eps, int relu) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cpg = C / 32, E = HW * cpg;
    const long base = (long)blockIdx.x * HW * C;
    for (int g = wave; g < 32; g += TPB / 64) {
        const float* q = x + base + g * cpg;
        double s = 0.0;
        for (int e = lane; e < E; e += 64) s += (double)q[(long)(e / cpg) * C + e % cpg];
        const double mean = wave_sum_d(s) / (double)E;
        double v = 0.0;
        for (int e = lane; e < E; e += 64) {
            const double d = (double)q[(long)(e / cpg) * C + e % cpg] - mean;
            v += d * d;
        }
        const double rstd = 1.0 / sqrt(wave_sum_d(v) / (double)E + eps);
        for (int e = lane; e < E; e += 64) {
            const int c = g * cpg + e % cpg;
            const long at = base + (long)(e / cpg) * C + c;
            float y = (float)(((double)x[at] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
            if (res) y = y + res[at];
            if (relu) y = fmaxf(y, 0.f);
            out[at] = y;
        }
    }
}

// MaxPool 3 x 3 / stride 2, 'SAME' (nothing in front, one behind, which a maximum ignores): [P][16][16][C] -> [P][8][8][C]
__global__ __launch_bounds__(TPB) void musiq_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int C, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ox = (int)(r % POOL_O);
    r /= POOL_O;
    const int oy = (int)(r % POOL_O);
    const long pt = r / POOL_O;
    float m = -INFINITY;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const int iy = 2 * oy + dy, ix = 2 * ox + dx;
            if (iy < STEM_O && ix < STEM_O) m = fmaxf(m, in[((pt * STEM_O + iy) * STEM_O + ix) * C + c]);
        }
    out[i] = m;
}

// x[img][0] = cls, x[img][1 + p] = (emb[img][p] + pos[hashed index of p]) + scale_emb[scale of p]
__global__ __launch_bounds__(TPB) void musiq_tokens_kernel(const float* __restrict__ emb, const float* __restrict__ pos, const float* __restrict__ semb,
                                                           const float* __restrict__ cls, IrMusiqLayout lay, int grid, int C, long total, float* __restrict__ x) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const long row = i / C;
    const int t = (int)(row % lay.T);
    const long im = row / lay.T;
    if (t == 0) {
        x[i] = cls[c];
        return;
    }
    const int pp = t - 1;
    int s = 0;
    while (s + 1 < lay.n_scales && pp >= lay.s[s + 1].first) ++s;
    const IrMusiqScale& g = lay.s[s];
    const int q = pp - g.first, gi = q / g.count_w, gj = q - gi * g.count_w;
    const int hi = min((int)floorf((float)gi * g.fh), grid - 1), wj = min((int)floorf((float)gj * g.fw), grid - 1);   // torch's nearest interpolation of arange(grid)
    const float e = emb[(im * lay.patches + pp) * C + c] + pos[(long)(hi * grid + wj) * C + c];
    x[i] = e + semb[(long)s * C + c];
}

// one wave per image: the final LayerNorm of the class token (feat: the fp64 value rounded once), then head_w . it + head_b
__global__ __launch_bounds__(64) void musiq_head_kernel(const float* __restrict__ x, long img_stride, int C, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, double eps, const float* __restrict__ hw, const float* __restrict__ hb, int n,
                                                        double* __restrict__ scores, float* __restrict__ feat) {
    const int im = blockIdx.x, lane = threadIdx.x;
    if (im >= n) return;
    const float* q = x + (long)im * img_stride;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)q[c];
    const double mean = wave_sum_d(s) / (double)C;
    double v = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)q[c] - mean;
        v += d * d;
    }
    const double rstd = 1.0 / sqrt(wave_sum_d(v) / (double)C + eps);
    double dot = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double y = ((double)q[c] - mean) * rstd * (double)gamma[c] + (double)beta[c];
        if (feat) feat[(long)im * C + c] = (float)y;
        dot += y * (double)hw[c];
    }
    dot = wave_sum_d(dot);
    if (lane == 0) scores[im] = dot + (double)hb[0];
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
    hipLaunchKernelGGL((musiq_gemm_kernel<AMODE, BMODE>), dim3((unsigned)((p.M + BM - 1) / BM), (unsigned)((p.N + BN - 1) / BN), (unsigned)z), dim3(TPB), 0, s, p);
}

}  // namespace

void ir_musiq_input_table_host(float* tab) {
    for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
        volatile float x = (float)v / 255.0f;
        volatile float y = x - 0.5f;
        tab[v] = y * 2.0f;
    }
}

int ir_musiq_layout_host(int h, int w, int patch, int grid, int n_scales, const int* longer, IrMusiqLayout* lay) {
    if (h < 1 || w < 1 || patch < 1 || grid < 1 || n_scales < 1 || n_scales > IR_MUSIQ_MAX_SCALES || !longer) return -1;
    long first = 0;
    lay->n_scales = n_scales;
    for (int k = 0; k < n_scales; ++k) {
        IrMusiqScale& g = lay->s[k];
        g.resized = longer[k] > 0;
        if (g.resized) {
            const double ratio = (double)longer[k] / (double)std::max(h, w);
            volatile double ph = (double)h * ratio, pw = (double)w * ratio;   // Python's round(h * ratio): half to even of the double product
            g.rh = (int)nearbyint(ph);
            g.rw = (int)nearbyint(pw);
        } else {
            g.rh = h;
            g.rw = w;
        }
        if (g.rh < 1 || g.rw < 1) return -1;
        g.count_h = (g.rh + patch - 1) / patch;
        g.count_w = (g.rw + patch - 1) / patch;
        g.pad_top = (g.count_h * patch - g.rh) / 2;
        g.pad_left = (g.count_w * patch - g.rw) / 2;
        g.first = (int)first;
        g.fh = (float)grid / (float)g.count_h;
        g.fw = (float)grid / (float)g.count_w;
        first += (long)g.count_h * g.count_w;
        if (first > (1L << 24)) return -1;
    }
    lay->patches = (int)first;
    lay->T = (int)first + 1;
    return 0;
}

int ir_musiq_plan(const IrMusiqModel& m, int n, int h, int w, IrMusiqPlan* pl) {
    if (n < 1 || n > 4096 || ir_musiq_layout_host(h, w, m.patch, m.grid, m.n_scales, m.longer, &pl->lay)) return -1;
    const size_t P = (size_t)n * pl->lay.patches, T = (size_t)pl->lay.T, C = (size_t)m.hidden;
    if ((double)P * STEM_O * STEM_O > 2.0e9 || (double)n * T * std::max(m.mlp, 3 * m.hidden) > 2.0e9 * TPB) return -1;   // M and every grid are ints
    pl->Tpad = (int)((T + BK - 1) / BK * BK);
    const size_t pair = T * pl->Tpad * sizeof(float);
    const size_t budget = std::max(SCORE_BYTES, std::min((size_t)m.heads * pair, SCORE_MAX));
    pl->zc = (int)std::min<size_t>(std::max<size_t>(budget / pair, 1), std::min<size_t>((size_t)n * m.heads, 32768));   // grid.z
    size_t at = 0;
    const size_t per[5] = {(size_t)STEM_O * STEM_O * STEM_C, (size_t)POOL_O * POOL_O * OUT_C, (size_t)POOL_O * POOL_O * STEM_C, (size_t)POOL_O * POOL_O * STEM_C,
                           (size_t)POOL_O * POOL_O * STEM_C};
    for (int k = 0; k < 5; ++k) {
        pl->slot[k] = at;
        at += up256(P * per[k] * sizeof(float));
    }
    size_t tr = 0;
    auto take = [&](size_t floats) {
        const size_t o = tr;
        tr += up256(floats * sizeof(float));
        return o;
    };
    pl->x = take((size_t)n * T * C);
    pl->hn = take((size_t)n * T * C);
    pl->qkv = take((size_t)n * T * 3 * C);
    pl->o = take((size_t)n * T * C);
    pl->f = take((size_t)n * T * m.mlp);
    pl->s = take((size_t)pl->zc * T * pl->Tpad);
    at = std::max(at, tr);
    pl->emb = at;
    at += up256(P * C * sizeof(float));
    pl->total = at;
    return 0;
}

int ir_launch_musiq(const IrMusiqModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws, hipStream_t s) {
    IrMusiqPlan pl;
    if (ir_musiq_plan(m, n, h, w, &pl)) return -1;
    char* base = static_cast<char*>(ws);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float *SA = at(pl.slot[0]), *SB = at(pl.slot[1]), *SC = at(pl.slot[2]), *SD = at(pl.slot[3]), *SE = at(pl.slot[4]), *emb = at(pl.emb);
    const int P = n * pl.lay.patches, T = pl.lay.T, C = m.hidden, HWs = STEM_O * STEM_O, HWp = POOL_O * POOL_O;
    static_assert(PIN <= POOL_O * POOL_O * OUT_C, "a patch's input lies in slot B");

    {   // every patch's input pixels -> SB
        PatchArgs p{};
        p.img = img; p.pitch = pitch; p.img_stride = (long)rows * pitch; p.h = h; p.w = w; p.tab = m.tab; p.lay = pl.lay;
        p.total = (long)P * PATCH * PATCH; p.out = SB;
        hipLaunchKernelGGL(musiq_patch_kernel, dim3(blocks_of(p.total, TPB)), dim3(TPB), 0, s, p);
    }
    {   // the stem: conv 7 x 7 / 2 -> SA, GroupNorm + ReLU in place, max-pool -> SC
        GemmArgs p = gemm_args(SB, 0, m.stem_w, STEM_C, P * HWs, STEM_C, STEM_K, nullptr, nullptr, SA, STEM_C);
        launch_gemm<A_STEM, B_KN>(p, 1, s);
        hipLaunchKernelGGL(musiq_gn_kernel, dim3(P), dim3(TPB), 0, s, SA, (const float*)nullptr, SA, HWs, STEM_C, m.stem_g, m.stem_b, 1e-6, 1);
        const long total = (long)P * HWp * STEM_C;
        hipLaunchKernelGGL(musiq_pool_kernel, dim3(blocks_of(total, TPB)), dim3(TPB), 0, s, SA, SC, STEM_C, total);
    }
    {   // the bottleneck: SC -> conv1 -> SD -> conv2 (3 x 3) -> SE -> conv3 -> SA; the projection SC -> SB; SA = relu(gn(SA) + gn(SB))
        const int M = P * HWp;
        GemmArgs p = gemm_args(SC, STEM_C, m.cw[0], STEM_C, M, STEM_C, STEM_C, nullptr, nullptr, SD, STEM_C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        hipLaunchKernelGGL(musiq_gn_kernel, dim3(P), dim3(TPB), 0, s, SD, (const float*)nullptr, SD, HWp, STEM_C, m.cg[0], m.cb[0], 1e-4, 1);
        p = gemm_args(SD, 0, m.cw[1], STEM_C, M, STEM_C, 9 * STEM_C, nullptr, nullptr, SE, STEM_C);
        p.H = POOL_O; p.W = POOL_O; p.cin = STEM_C;
        launch_gemm<A_CONV3, B_KN>(p, 1, s);
        hipLaunchKernelGGL(musiq_gn_kernel, dim3(P), dim3(TPB), 0, s, SE, (const float*)nullptr, SE, HWp, STEM_C, m.cg[1], m.cb[1], 1e-4, 1);
        p = gemm_args(SE, STEM_C, m.cw[2], OUT_C, M, OUT_C, STEM_C, nullptr, nullptr, SA, OUT_C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        p = gemm_args(SC, STEM_C, m.cw[3], OUT_C, M, OUT_C, STEM_C, nullptr, nullptr, SB, OUT_C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        hipLaunchKernelGGL(musiq_gn_kernel, dim3(P), dim3(TPB), 0, s, SB, (const float*)nullptr, SB, HWp, OUT_C, m.cg[3], m.cb[3], 1e-4, 0);
        hipLaunchKernelGGL(musiq_gn_kernel, dim3(P), dim3(TPB), 0, s, SA, (const float*)SB, SA, HWp, OUT_C, m.cg[2], m.cb[2], 1e-4, 1);
    }
    {   // the embedding of the (y, x, c) flattened map - the NHWC map as it lies - and the tokens (x lies over the slots, emb does not)
        const int K = HWp * OUT_C;
        GemmArgs p = gemm_args(SA, K, m.emb_w, C, P, C, K, m.emb_b, nullptr, emb, C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
    }
    float *X = at(pl.x), *HN = at(pl.hn), *QKV = at(pl.qkv), *O = at(pl.o), *F = at(pl.f), *S = at(pl.s);
    const long R = (long)n * T;
    hipLaunchKernelGGL(musiq_tokens_kernel, dim3(blocks_of(R * C, TPB)), dim3(TPB), 0, s, emb, m.pos, m.semb, m.cls, pl.lay, m.grid, C, R * C, X);
    const int pairs = n * m.heads, hd = C / m.heads;
    for (int l = 0; l < m.layers; ++l) {
        const IrMusiqBlock& b = m.blk[l];
        launch_ln(X, R, C, b.ln1g, b.ln1b, 1e-6, HN, s);
        GemmArgs p = gemm_args(HN, C, b.qkvw, 3 * C, (int)R, 3 * C, C, b.qkvb, nullptr, QKV, 3 * C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        for (int z0 = 0; z0 < pairs; z0 += pl.zc) {
            const int z = std::min(pl.zc, pairs - z0);
            p = gemm_args(QKV, 3 * C, QKV + C, 3 * C, T, T, hd, nullptr, nullptr, S, pl.Tpad);   // q k^T / sqrt(hd)
            p.alpha = 1.0f / sqrtf((float)hd);
            p.z0 = z0; p.zdiv = m.heads;
            p.a_s0 = p.b_s0 = (long)T * 3 * C; p.a_s1 = p.b_s1 = hd; p.c_sl = (long)T * pl.Tpad;
            launch_gemm<A_ROWS, B_NK>(p, z, s);
            launch_softmax(S, (long)z * T, T, pl.Tpad, s);
            p = gemm_args(S, pl.Tpad, QKV + 2 * C, 3 * C, T, hd, pl.Tpad, nullptr, nullptr, O, C);   // p v; the padded columns of p are 0
            p.Kb = T;
            p.z0 = z0; p.zdiv = m.heads;
            p.a_sl = (long)T * pl.Tpad; p.b_s0 = (long)T * 3 * C; p.b_s1 = hd; p.c_s0 = (long)T * C; p.c_s1 = hd;
            launch_gemm<A_ROWS, B_KN>(p, z, s);
        }
        p = gemm_args(O, C, b.ow, C, (int)R, C, C, b.ob, X, X, C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        launch_ln(X, R, C, b.ln2g, b.ln2b, 1e-6, HN, s);
        p = gemm_args(HN, C, b.f1w, m.mlp, (int)R, m.mlp, C, b.f1b, nullptr, F, m.mlp);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
        launch_gelu(F, R * m.mlp, s);
        p = gemm_args(F, m.mlp, b.f2w, C, (int)R, C, m.mlp, b.f2b, X, X, C);
        launch_gemm<A_ROWS, B_KN>(p, 1, s);
    }
    hipLaunchKernelGGL(musiq_head_kernel, dim3(n), dim3(64), 0, s, X, (long)T * C, C, m.fin_g, m.fin_b, 1e-6, m.head_w, m.head_b, n, scores, feat);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
