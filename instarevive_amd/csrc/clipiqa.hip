// CLIP-IQA of uint8 HWC RGB device images (ir_clipiqa): the model of tools/evaluate_clipiqa.py - CLIP's ModifiedResNet image tower at the image's
// own size, its attention pool without positional embedding, and the pair softmax against the fixed text rows - in exact fp32 with an fp64 tail.
//   Convolutions: implicit GEMMs on the exact-fp32 tile loop of exact_f32_tile.h, NHWC fp32 maps, M = output pixels of the n images, N = cout,
//   K = k * k * cin in (ky, kx, c) order with the weights repacked to [K padded to 32][cout] by ir_clipiqa_configure. One kernel serves 1 x 1 and
//   3 x 3 at stride 1 (cin and cout multiples of 32: a 32-deep k-tile never crosses a tap); the tile is 128 x BN (BN = 128 / 64 / 32 by cout's
//   largest such divisor), or 64 x 64 where the larger one would leave fewer than 512 workgroups.
//   Epilogue: acc * scale[c] + shift[c] (the BatchNorm folded in fp64 and rounded once), an optional residual add, an optional ReLU -
//   separate roundings, the file is built with -ffp-contract=off. The 3-channel stride-2 stem conv
//   gathers from the bytes through the 3 x 256 table (the host's fp32 (v / 255 - mean) / std), K = 27 padded to 32; padding is 0 in that domain.
//   AvgPool2d(2), floor mode, is a kernel of its own: ((a + b) + (c + d)) * 0.25.
//   Tail, all fp64, one image per grid.y: the token mean; q = (Wq x0 + bq) hd^-0.5 for the one query that is used; since only that query
//   exists, its scores are u_h . x_t + q_h . bk_h with u_h = Wk_h^T q_h, and the attention output is Wv_h (sum_t p_th x_t) + bv_h (the p sum
//   to 1) - algebraically the three projections, at T C heads instead of T C C multiplies; softmax over the T = HW + 1 tokens; c_proj; the
//   feature norm, the logits against the text rows, the softmax of each pair, the mean of the first entries. Every sum is a per-thread or
//   per-lane sequential chain followed by a fixed butterfly / a fixed fold: the same bits on every call and at every
//   place in a batch. One double per image.
// Reads are clipped to the scored rectangle h x w; every store is guarded by the row count of its launch.
#include <algorithm>

#include "common.h"
#include "exact_f32_tile.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int SMALL_GRID = 512;   // below this many 128-row workgroups a launch takes the 64 x 64 tile: two or more workgroups per CU hide the k-tile's latency

struct ConvArgs {
    // stem: the byte images
    const uint8_t* img;
    long pitch, img_stride;
    const float* tab;           // [3][256]
    // else: an NHWC fp32 map
    const float* in;            // [imgs][H][W][cin]
    int H, W, cin;              // input size (stem: the byte image's h, w)
    int Ho, Wo, ks, pad;
    int M, K, N;                // M = imgs * Ho * Wo, K = ks * ks * cin (un-padded), N = cout
    const float* wgt;           // [Kpad][N]
    const float *scale, *shift; // [N]
    const float* res;           // [M][N] or null
    int relu;
    float* out;                 // [M][N]
};

// folded BatchNorm, residual, ReLU
struct BnResRelu {
    const ConvArgs& p;
    int col;
    float sc, sh;
    IR_DEVINL bool column(int c) {
        col = c;
        sc = p.scale[c];
        sh = p.shift[c];
        return true;   // N is a multiple of BN
    }
    IR_DEVINL void store(int m, float acc) const {
        float v = acc * sc + sh;
        if (p.res) v = v + p.res[(long)m * p.N + col];
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[(long)m * p.N + col] = v;
    }
};

// STEM: 3 x 3 / stride 2 / pad 1 from the bytes through the table; else stride 1 from an fp32 map whose cin is a multiple of BK
template <int BM, int BN, bool STEM>
__global__ __launch_bounds__(TPB, STEM ? (BN == 64 ? 3 : 4) : BM == 64 ? 7 : BN == 128 ? 3 : BN == 64 ? 4 : 6) void clipiqa_conv_kernel(ConvArgs p) {
    const KnB<BN, false> b{.b = p.wgt, .ldb = p.N};
    if constexpr (STEM) {
        __shared__ float s_tab[3 * 256];
        const ByteTableA<BM, false> a{.a = p.img, .a_pitch = p.pitch, .a_img = p.img_stride, .tab = p.tab, .s_tab = s_tab, .H = p.H, .W = p.W, .Ho = p.Ho, .Wo = p.Wo,
                                      .row_k = 9, .stride = 2, .pad = p.pad, .M = p.M, .K = p.K};   // 9 = 3 taps x 3 channels of one image row
        tile_loop<BM, BN>(a, b, p.M, p.K, BnResRelu{p});
    } else {
        const NhwcA<BM, true> a{.in = p.in, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.cin, .kw = p.ks, .stride = 1, .ph = p.pad, .pw = p.pad, .Ho = p.Ho, .Wo = p.Wo, .M = p.M, .K = p.K};
        tile_loop<BM, BN>(a, b, p.M, p.K, BnResRelu{p});
    }
}

// AvgPool2d(2), floor mode: Ho = H / 2, an odd trailing row or column is dropped
__global__ __launch_bounds__(TPB) void clipiqa_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int Ho, int Wo, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const long img = r / Ho;
    const float* q = in + ((img * H + 2 * oy) * W + 2 * ox) * C + c;
    out[i] = ((q[0] + q[C]) + (q[(long)W * C] + q[(long)W * C + C])) * 0.25f;
}

IR_DEVINL double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// x0[img][c] = (sum over the HW tokens) / HW. A workgroup takes 32 channels; token group g of 8 sums tokens g, g + 8, ... in order, the eight
// partial sums are added in order of g.
__global__ __launch_bounds__(TPB) void clipiqa_mean_kernel(const float* __restrict__ x, int HW, int C, double* __restrict__ x0) {
    __shared__ double s_part[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    double s = 0.0;
    if (c < C) {
        const float* q = x + (long)blockIdx.y * HW * C + c;
        for (int t = g; t < HW; t += 8) s += (double)q[(long)t * C];
    }
    s_part[g][cl] = s;
    __syncthreads();
    if (g == 0 && c < C) {
        double r = s_part[0][cl];
#pragma unroll
        for (int i = 1; i < 8; ++i) r += s_part[i][cl];
        x0[(long)blockIdx.y * C + c] = r / (double)HW;
    }
}

// out[img][j] = (W[j] . vec[img][j / group] + b[j]) * mul for j < rows: one wave per row; vec: [imgs][rows / group][cols] doubles
__global__ __launch_bounds__(TPB) void clipiqa_gemv_kernel(const float* __restrict__ W, const float* __restrict__ b, const double* __restrict__ vec, int rows, int cols,
                                                           int group, double mul, double* __restrict__ out, float* __restrict__ outf) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (j >= rows) return;   // uniform over the wave
    const double* v = vec + ((long)blockIdx.y * (rows / group) + j / group) * cols;
    const float* w = W + (long)j * cols;
    double s = 0.0;
    for (int c = lane; c < cols; c += 64) s += (double)w[c] * v[c];
    s = wave_sum_d(s);
    if (lane == 0) {
        const double r = (s + (double)b[j]) * mul;
        out[(long)blockIdx.y * rows + j] = r;
        if (outf) outf[(long)blockIdx.y * rows + j] = (float)r;
    }
}

// u[img][h][c] = sum_d Wk[h hd + d][c] q[img][h hd + d], c0[img][h] = sum_d q[img][h hd + d] bk[h hd + d]
__global__ __launch_bounds__(TPB) void clipiqa_qk_kernel(const float* __restrict__ Wk, const float* __restrict__ bk, const double* __restrict__ q, int C, int hd, int heads,
                                                         double* __restrict__ u, double* __restrict__ c0) {
    const int c = blockIdx.x * TPB + threadIdx.x, h = blockIdx.y;
    if (c >= C) return;
    const double* qh = q + (long)blockIdx.z * C + h * hd;
    double s = 0.0;
    for (int d = 0; d < hd; ++d) s += (double)Wk[(long)(h * hd + d) * C + c] * qh[d];
    u[((long)blockIdx.z * heads + h) * C + c] = s;
    if (c == 0) {
        double t = 0.0;
        for (int d = 0; d < hd; ++d) t += qh[d] * (double)bk[h * hd + d];
        c0[(long)blockIdx.z * heads + h] = t;
    }
}

// s[img][t][h] = u[img][h] . x_t + c0[img][h]; token 0 is the mean token (fp64), token t > 0 the map's pixel t - 1. A wave takes TPW tokens
// and the HPG heads of group blockIdx.z.
constexpr int TPW = 4, HPG = 4;
__global__ __launch_bounds__(TPB) void clipiqa_scores_kernel(const float* __restrict__ x, const double* __restrict__ x0, const double* __restrict__ u,
                                                             const double* __restrict__ c0, int T, int C, int heads, double* __restrict__ s) {
    const int lane = threadIdx.x & 63, img = blockIdx.y;
    const int t0 = (blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)) * TPW;
    if (t0 >= T) return;   // uniform over the wave
    const float* xi = x + (long)img * (T - 1) * C;
    const double* x0i = x0 + (long)img * C;
    const int h1 = min((int)(blockIdx.z + 1) * HPG, heads);
    for (int h = blockIdx.z * HPG; h < h1; ++h) {
        const double* uh = u + ((long)img * heads + h) * C;
        double acc[TPW];
#pragma unroll
        for (int k = 0; k < TPW; ++k) acc[k] = 0.0;
        for (int c = lane; c < C; c += 64) {
            const double uu = uh[c];
#pragma unroll
            for (int k = 0; k < TPW; ++k) {
                const int t = t0 + k;
                if (t < T) acc[k] += uu * (t == 0 ? x0i[c] : (double)xi[(long)(t - 1) * C + c]);
            }
        }
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            const double r = wave_sum_d(acc[k]);
            if (lane == 0 && t0 + k < T) s[((long)img * T + t0 + k) * heads + h] = r + c0[(long)img * heads + h];
        }
    }
}

// softmax over the tokens of head blockIdx.x of image blockIdx.y, in place
__global__ __launch_bounds__(TPB) void clipiqa_softmax_kernel(double* __restrict__ s, int T, int heads) {
    __shared__ double s_red[TPB / 64];
    double* q = s + (long)blockIdx.y * T * heads + blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = -1.0e300;
    for (int t = threadIdx.x; t < T; t += TPB) mx = fmax(mx, q[(long)t * heads]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int i = 1; i < TPB / 64; ++i) mx = fmax(mx, s_red[i]);
    __syncthreads();
    double sum = 0.0;
    for (int t = threadIdx.x; t < T; t += TPB) {
        const double e = exp(q[(long)t * heads] - mx);
        q[(long)t * heads] = e;
        sum += e;
    }
    sum = wave_sum_d(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    sum = s_red[0];
#pragma unroll
    for (int i = 1; i < TPB / 64; ++i) sum += s_red[i];
    for (int t = threadIdx.x; t < T; t += TPB) q[(long)t * heads] = q[(long)t * heads] / sum;
}

// y[img][h][c] = sum_t p[img][t][h] x_t[c]. A workgroup takes 32 channels of one head; token group g of 8 sums tokens g, g + 8, ... in order
// (token 0 is the mean token), the eight partial sums are added in order of g.
__global__ __launch_bounds__(TPB) void clipiqa_mix_kernel(const float* __restrict__ x, const double* __restrict__ x0, const double* __restrict__ p, int T, int C, int heads,
                                                          double* __restrict__ y) {
    __shared__ double s_part[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl, h = blockIdx.y, img = blockIdx.z;
    double s = 0.0;
    if (c < C) {
        const float* xi = x + (long)img * (T - 1) * C + c;
        const double* pi = p + (long)img * T * heads + h;
        if (g == 0) s = pi[0] * x0[(long)img * C + c];
        for (int t = g == 0 ? 8 : g; t < T; t += 8) s += pi[(long)t * heads] * (double)xi[(long)(t - 1) * C];
    }
    s_part[g][cl] = s;
    __syncthreads();
    if (g == 0 && c < C) {
        double r = s_part[0][cl];
#pragma unroll
        for (int i = 1; i < 8; ++i) r += s_part[i][cl];
        y[((long)img * heads + h) * C + c] = r;
    }
}

// one wave per image: f / |f|, the logits against the 2 * pairs text rows, the softmax of every pair, the mean of the first entries
__global__ __launch_bounds__(64) void clipiqa_score_kernel(const double* __restrict__ f, const float* __restrict__ text, int D, int pairs, double logit_scale, int n,
                                                           double* __restrict__ out) {
    const int img = blockIdx.x, lane = threadIdx.x;
    if (img >= n) return;
    const double* fi = f + (long)img * D;
    double nn = 0.0;
    for (int c = lane; c < D; c += 64) nn += fi[c] * fi[c];
    const double norm = sqrt(wave_sum_d(nn));
    double total = 0.0;
    for (int k = 0; k < pairs; ++k) {
        double a = 0.0, b = 0.0;
        for (int c = lane; c < D; c += 64) {
            const double v = fi[c] / norm;
            a += (double)text[(long)(2 * k) * D + c] * v;
            b += (double)text[(long)(2 * k + 1) * D + c] * v;
        }
        a = logit_scale * wave_sum_d(a);
        b = logit_scale * wave_sum_d(b);
        const double mx = fmax(a, b), ea = exp(a - mx), eb = exp(b - mx);
        total += ea / (ea + eb);
    }
    if (lane == 0) out[img] = total / (double)pairs;
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

void launch_conv(const IrClipConv& cv, const float* in, const float* res, int relu, float* out, int imgs, int H, int W, hipStream_t s) {
    ConvArgs p{};
    p.in = in; p.H = H; p.W = W; p.cin = cv.cin;
    p.Ho = H; p.Wo = W; p.ks = cv.ks; p.pad = cv.ks / 2;
    p.M = imgs * H * W; p.K = cv.ks * cv.ks * cv.cin; p.N = cv.cout;
    p.wgt = cv.w; p.scale = cv.scale; p.shift = cv.shift; p.res = res; p.relu = relu; p.out = out;
    const unsigned gm = (unsigned)((p.M + 127) / 128), gs = (unsigned)((p.M + 63) / 64);
    const int bn = cv.cout % 128 == 0 ? 128 : cv.cout % 64 == 0 ? 64 : 32;
    // the tile does not change a single output (a k-ordered chain each): it is chosen for the grid alone
    if (bn >= 64 && (long)gm * (cv.cout / bn) < SMALL_GRID)
        hipLaunchKernelGGL((clipiqa_conv_kernel<64, 64, false>), dim3(gs, cv.cout / 64), dim3(TPB), 0, s, p);
    else if (bn == 128)
        hipLaunchKernelGGL((clipiqa_conv_kernel<128, 128, false>), dim3(gm, cv.cout / 128), dim3(TPB), 0, s, p);
    else if (bn == 64)
        hipLaunchKernelGGL((clipiqa_conv_kernel<128, 64, false>), dim3(gm, cv.cout / 64), dim3(TPB), 0, s, p);
    else
        hipLaunchKernelGGL((clipiqa_conv_kernel<128, 32, false>), dim3(gm, cv.cout / 32), dim3(TPB), 0, s, p);
}

void launch_pool(const float* in, float* out, int imgs, int H, int W, int C, hipStream_t s) {
    const long total = (long)imgs * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(clipiqa_pool_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, in, out, H, W, C, H / 2, W / 2, total);
}

}  // namespace

int ir_clipiqa_plan(const IrClipiqaModel& m, int n, int h, int w, IrClipiqaPlan* pl) {
    if (n < 1 || n > 65535 || h < 32 || w < 32) return -1;
    size_t fl[5] = {0, 0, 0, 0, 0};   // floats per image of the five map slots
    int H = (h - 1) / 2 + 1, W = (w - 1) / 2 + 1;
    if ((double)n * H * W > 2.0e9) return -1;   // M is an int
    fl[0] = (size_t)H * W * std::max(m.stem[0].cout, m.stem[2].cout);
    fl[1] = (size_t)H * W * m.stem[1].cout;
    H /= 2;
    W /= 2;
    fl[1] = std::max(fl[1], (size_t)H * W * m.stem[2].cout);
    int cur = 1;
    for (int i = 0; i < m.n_blocks; ++i) {
        const IrClipBlock& b = m.blocks[i];
        const int Ho = b.stride == 2 ? H / 2 : H, Wo = b.stride == 2 ? W / 2 : W;
        if (Ho < 1 || Wo < 1) return -1;
        if (b.has_down) {
            if (b.stride == 2) fl[2] = std::max(fl[2], (size_t)Ho * Wo * b.c1.cin);
            fl[4] = std::max(fl[4], (size_t)Ho * Wo * b.c3.cout);
        }
        fl[2] = std::max(fl[2], (size_t)H * W * b.c1.cout);
        fl[3] = std::max(fl[3], (size_t)H * W * b.c2.cout);
        fl[1 - cur] = std::max(fl[1 - cur], (size_t)Ho * Wo * b.c3.cout);
        cur = 1 - cur;
        H = Ho;
        W = Wo;
    }
    pl->fh = H;
    pl->fw = W;
    pl->final_slot = cur;
    size_t at = 0;
    for (int k = 0; k < 5; ++k) {
        pl->slot[k] = at;
        at += up256((size_t)n * fl[k] * sizeof(float));
    }
    const size_t C = (size_t)m.width * 32, T = (size_t)H * W + 1, hd = m.heads;
    // x0, q, u, c0, p, y, a, f
    const size_t cnt[8] = {C, C, hd * C, hd, T * hd, hd * C, C, (size_t)m.out_dim};
    for (int k = 0; k < 8; ++k) {
        pl->tail[k] = at;
        at += up256((size_t)n * cnt[k] * sizeof(double));
    }
    pl->total = at;
    return 0;
}

int ir_launch_clipiqa(const IrClipiqaModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws, hipStream_t s) {
    IrClipiqaPlan pl;
    if (ir_clipiqa_plan(m, n, h, w, &pl)) return -1;
    char* base = static_cast<char*>(ws);
    float* S[5];
    for (int k = 0; k < 5; ++k) S[k] = reinterpret_cast<float*>(base + pl.slot[k]);
    double* D[8];
    for (int k = 0; k < 8; ++k) D[k] = reinterpret_cast<double*>(base + pl.tail[k]);

    int H = (h - 1) / 2 + 1, W = (w - 1) / 2 + 1;
    {   // the stem: conv (bytes) -> S0, conv -> S1, conv -> S0, pool -> S1
        const IrClipConv& cv = m.stem[0];
        ConvArgs p{};
        p.img = img; p.pitch = pitch; p.img_stride = (long)rows * pitch; p.tab = m.tab;
        p.H = h; p.W = w; p.cin = 3; p.Ho = H; p.Wo = W; p.ks = 3; p.pad = 1;
        p.M = n * H * W; p.K = 27; p.N = cv.cout;
        p.wgt = cv.w; p.scale = cv.scale; p.shift = cv.shift; p.res = nullptr; p.relu = 1; p.out = S[0];
        const unsigned gm = (unsigned)((p.M + 127) / 128);
        if (cv.cout % 64 == 0)
            hipLaunchKernelGGL((clipiqa_conv_kernel<128, 64, true>), dim3(gm, cv.cout / 64), dim3(TPB), 0, s, p);
        else
            hipLaunchKernelGGL((clipiqa_conv_kernel<128, 32, true>), dim3(gm, cv.cout / 32), dim3(TPB), 0, s, p);
        launch_conv(m.stem[1], S[0], nullptr, 1, S[1], n, H, W, s);
        launch_conv(m.stem[2], S[1], nullptr, 1, S[0], n, H, W, s);
        launch_pool(S[0], S[1], n, H, W, m.stem[2].cout, s);
        H /= 2;
        W /= 2;
    }
    int cur = 1;
    for (int i = 0; i < m.n_blocks; ++i) {
        const IrClipBlock& b = m.blocks[i];
        const int Ho = b.stride == 2 ? H / 2 : H, Wo = b.stride == 2 ? W / 2 : W;
        const float* x = S[cur];
        const float* idn = x;
        if (b.has_down) {   // identity first, so that S2 is free for the main branch
            const float* src = x;
            if (b.stride == 2) {
                launch_pool(x, S[2], n, H, W, b.c1.cin, s);
                src = S[2];
            }
            launch_conv(b.down, src, nullptr, 0, S[4], n, Ho, Wo, s);
            idn = S[4];
        }
        launch_conv(b.c1, x, nullptr, 1, S[2], n, H, W, s);
        launch_conv(b.c2, S[2], nullptr, 1, S[3], n, H, W, s);
        const float* t2 = S[3];
        if (b.stride == 2) {
            launch_pool(S[3], S[2], n, H, W, b.c2.cout, s);
            t2 = S[2];
        }
        launch_conv(b.c3, t2, idn, 1, S[1 - cur], n, Ho, Wo, s);
        cur = 1 - cur;
        H = Ho;
        W = Wo;
    }

    const float* x = S[cur];
    const int C = m.width * 32, heads = m.heads, hd = C / heads, HW = H * W, T = HW + 1, OD = m.out_dim;
    double *x0 = D[0], *q = D[1], *u = D[2], *c0 = D[3], *p = D[4], *y = D[5], *a = D[6], *f = D[7];
    const unsigned gc = (unsigned)((C + TPB - 1) / TPB), gr = (unsigned)((C + 3) / 4), g32 = (unsigned)((C + 31) / 32);
    hipLaunchKernelGGL(clipiqa_mean_kernel, dim3(g32, n), dim3(TPB), 0, s, x, HW, C, x0);
    hipLaunchKernelGGL(clipiqa_gemv_kernel, dim3(gr, n), dim3(TPB), 0, s, m.qw, m.qb, x0, C, C, C, 1.0 / sqrt((double)hd), q, (float*)nullptr);
    hipLaunchKernelGGL(clipiqa_qk_kernel, dim3(gc, heads, n), dim3(TPB), 0, s, m.kw, m.kb, q, C, hd, heads, u, c0);
    hipLaunchKernelGGL(clipiqa_scores_kernel, dim3((unsigned)((T + 4 * TPW - 1) / (4 * TPW)), n, (unsigned)((heads + HPG - 1) / HPG)), dim3(TPB), 0, s, x, x0, u, c0, T, C, heads, p);
    hipLaunchKernelGGL(clipiqa_softmax_kernel, dim3(heads, n), dim3(TPB), 0, s, p, T, heads);
    hipLaunchKernelGGL(clipiqa_mix_kernel, dim3(g32, heads, n), dim3(TPB), 0, s, x, x0, p, T, C, heads, y);
    hipLaunchKernelGGL(clipiqa_gemv_kernel, dim3(gr, n), dim3(TPB), 0, s, m.vw, m.vb, y, C, C, hd, 1.0, a, (float*)nullptr);
    hipLaunchKernelGGL(clipiqa_gemv_kernel, dim3((unsigned)((OD + 3) / 4), n), dim3(TPB), 0, s, m.cw, m.cb, a, OD, C, OD, 1.0, f, feat);
    hipLaunchKernelGGL(clipiqa_score_kernel, dim3(n), dim3(64), 0, s, f, m.text, OD, m.n_pairs, m.logit_scale, n, scores);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
