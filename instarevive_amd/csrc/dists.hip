// DISTS of uint8 HWC RGB device images (ir_dists): the model of tools/evaluate_pairs.py::DISTS, exact fp32 convolutions and fp64 statistics.
// The 2n images of a call (a's n, then b's n) go through one set of launches:
//   the thirteen 3x3 convolutions of VGG-16 as implicit GEMMs on the exact-fp32 tile loop of exact_f32_tile.h, bias + ReLU in the epilogue,
//   feature maps NHWC fp32. M = pixels of 2n images, N = cout, K = 9 cin in (ky, kx, c) order - the weights are repacked to
//   [K padded to 32][cout] by ir_dists_configure, zero rows behind K (27 -> 32 for the first conv; the A tile is zero there as well). The tile
//   is 128 x BN, BN = 128 where cout is a multiple of 128, else 64. The first conv gathers straight from the bytes through the 3 x 256 table
//   (the host's fp32 (v / 255 - mean) / std, so the network's input is the host model's to the bit); padding is 0 in that normalised domain.
//   The L2 pool in front of stages 2 .. 5 is one kernel: sqrt(sum_taps g x^2 + 1e-12), g = (1, 2, 1) x (1, 2, 1) / 16, stride 2, padding 1,
//   the taps added row by row from the top-left in fp32 (the file is built with -ffp-contract=off); taps outside the map add nothing.
//   One moment kernel per compared map: a lane per channel, 1024 pixels per workgroup, the five sums of a pair in fp64 about the channel's
//   first pixel (sum dx, sum dy, sum dx^2, sum dy^2, sum dx dy with dx = x - x[0]: a constant map sums to exactly 0), the workgroup's sums to
//   the workspace; a fold kernel adds the partials of a (pair, channel) in a fixed order and writes mx, my, vx, vy, cxy; the last launch makes
//   S1, S2 and the weighted sum of a pair in fp64: a pair gives the same bits on every call and at every place in a batch.
// Reads are clipped to the compared rectangle h x w of either image; every store is guarded by the row count M of its launch.
#include <algorithm>

#include "common.h"
#include "exact_f32_tile.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int BM = 128;
constexpr int MOM_PIX = 1024;   // pixels per workgroup of the moment kernels: the unit of the partial sums

struct ConvArgs {
    // input: the byte images (first conv) or an NHWC fp32 map
    const uint8_t *a, *b;
    long a_pitch, a_img, b_pitch, b_img;
    int n;                      // images of a (the following n are b's)
    const float* tab;           // [3][256] input table
    const float* in;            // [imgs][H][W][cin]
    int H, W, cin;              // map size (3x3, stride 1, padding 1: the output's as well)
    int M, K, N;                // M = imgs * H * W, K = 9 * cin (un-padded), N = cout
    const float* wgt;           // [Kpad][N]
    const float* bias;          // [N]
    float* out;                 // [M][N]
};

struct BiasRelu {
    const ConvArgs& p;
    int col;
    float bias;
    IR_DEVINL bool column(int c) {
        col = c;
        bias = p.bias[c];
        return true;   // N is a multiple of BN
    }
    IR_DEVINL void store(int m, float acc) const { p.out[(long)m * p.N + col] = fmaxf(acc + bias, 0.f); }
};

// FIRST: the first conv (bytes through the table, K = 27); else from an fp32 map whose cin is a multiple of BK. Waves per SIMD: the 128 x 128
// tile asks for one, which leaves its accumulators in AGPRs at two waves - DISTS's large maps run it at the MFMA rate, where that measured faster
// than VGPR accumulators at three (docs/kernels.md)
template <int BN, bool FIRST>
__global__ __launch_bounds__(TPB, FIRST ? 2 : BN == 128 ? 1 : 4) void dists_conv_kernel(ConvArgs p) {
    const KnB<BN, false> b{.b = p.wgt, .ldb = p.N};
    if constexpr (FIRST) {
        __shared__ float s_tab[3 * 256];
        const ByteTableA<BM, true> a{.a = p.a, .b = p.b, .a_pitch = p.a_pitch, .a_img = p.a_img, .b_pitch = p.b_pitch, .b_img = p.b_img, .n = p.n, .tab = p.tab, .s_tab = s_tab,
                                     .H = p.H, .W = p.W, .Ho = p.H, .Wo = p.W, .row_k = 9, .stride = 1, .pad = 1, .M = p.M, .K = p.K};   // 9 = 3 taps x 3 channels of one image row
        tile_loop<BM, BN>(a, b, p.M, p.K, BiasRelu{p});
    } else {
        const NhwcA<BM, true> a{.in = p.in, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.cin, .kw = 3, .stride = 1, .ph = 1, .pw = 1, .Ho = p.H, .Wo = p.W, .M = p.M, .K = p.K};
        tile_loop<BM, BN>(a, b, p.M, p.K, BiasRelu{p});
    }
}

// L2 pool: in [imgs][H][W][C] -> out [imgs][Ho][Wo][C], Ho = ceil(H / 2); a thread per four channels of an output pixel (C4 = C / 4)
__global__ __launch_bounds__(TPB) void dists_pool_kernel(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4, int Ho, int Wo, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    long r = i / C4;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const long img = r / Ho;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = 2 * oy - 1 + dy;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = 2 * ox - 1 + dx;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;   // a tap outside the map contributes 0
            const float g = (dy == 1 ? 0.5f : 0.25f) * (dx == 1 ? 0.5f : 0.25f);
            const float4 v = in[((img * H + iy) * W + ix) * C4 + c];
            s.x = s.x + g * (v.x * v.x);
            s.y = s.y + g * (v.y * v.y);
            s.z = s.z + g * (v.z * v.z);
            s.w = s.w + g * (v.w * v.w);
        }
    }
    out[i] = make_float4(__fsqrt_rn(s.x + 1e-12f), __fsqrt_rn(s.y + 1e-12f), __fsqrt_rn(s.z + 1e-12f), __fsqrt_rn(s.w + 1e-12f));
}

// feat: [2n][HW][C]; workgroup (x, y, z): pixels MOM_PIX * x .. of channels 64 y .. 64 y + 63 of pair z, a lane per channel, the waves' sums
// added in wave order; part: [n][chunks][C][5]
__global__ __launch_bounds__(TPB) void dists_moments_kernel(const float* __restrict__ feat, int n, int HW, int C, double* __restrict__ part) {
    __shared__ double s_red[TPB / 64][5][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane, pair = blockIdx.z;
    const float* fa = feat + (long)pair * HW * C + c;
    const float* fb = feat + (long)(pair + n) * HW * C + c;
    const double ka = (double)fa[0], kb = (double)fb[0];   // the pivots: the channel's first pixel
    const int p0 = blockIdx.x * MOM_PIX, p1 = min(HW, p0 + MOM_PIX);
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = p0 + wave; q < p1; q += TPB / 64) {
        const double x = (double)fa[(long)q * C] - ka, y = (double)fb[(long)q * C] - kb;
        s[0] += x;
        s[1] += y;
        s[2] += x * x;
        s[3] += y * y;
        s[4] += x * y;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) s_red[wave][j][lane] = s[j];
    __syncthreads();
    if (wave == 0) {
        double* q = part + (((long)pair * gridDim.x + blockIdx.x) * C + c) * 5;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double v = s_red[0][j][lane];
#pragma unroll
            for (int k = 1; k < TPB / 64; ++k) v += s_red[k][j][lane];
            q[j] = v;
        }
    }
}

struct RawArgs {
    const uint8_t *a, *b;
    long a_pitch, a_img, b_pitch, b_img;
    const float* x01;   // [256] (float)v / 255.0f
    int w, HW;
};

// map 0, the raw x = v / 255 of the bytes: workgroup (x, 0, z) = pixels MOM_PIX * x .. of pair z, a thread per pixel (four rounds); part: [n][chunks][3][5]
__global__ __launch_bounds__(TPB) void dists_raw_moments_kernel(RawArgs p, double* __restrict__ part) {
    __shared__ double s_red[TPB / 64][15];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.z;
    const uint8_t* pa = p.a + (long)pair * p.a_img;
    const uint8_t* pb = p.b + (long)pair * p.b_img;
    double ka[3], kb[3], s[15];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ka[c] = (double)p.x01[pa[c]];
        kb[c] = (double)p.x01[pb[c]];
    }
#pragma unroll
    for (int j = 0; j < 15; ++j) s[j] = 0.0;
    const int p0 = blockIdx.x * MOM_PIX, p1 = min(p.HW, p0 + MOM_PIX);
    for (int q = p0 + threadIdx.x; q < p1; q += TPB) {
        const int y = q / p.w, x = q - y * p.w;
        const uint8_t* qa = pa + (long)y * p.a_pitch + 3L * x;
        const uint8_t* qb = pb + (long)y * p.b_pitch + 3L * x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double u = (double)p.x01[qa[c]] - ka[c], v = (double)p.x01[qb[c]] - kb[c];
            s[5 * c] += u;
            s[5 * c + 1] += v;
            s[5 * c + 2] += u * u;
            s[5 * c + 3] += v * v;
            s[5 * c + 4] += u * v;
        }
    }
#pragma unroll
    for (int j = 0; j < 15; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o);
        if (lane == 0) s_red[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 15) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < TPB / 64; ++k) v += s_red[k][threadIdx.x];
        part[((long)pair * gridDim.x + blockIdx.x) * 15 + threadIdx.x] = v;
    }
}

// workgroup (c, pair): the partials of channel c added in a fixed order; mom[pair][choff + c] = (mx, my, vx, vy, cxy).
// The pivots are read again from where the moment kernel read them: feat (a map) or, when it is null, the bytes.
__global__ __launch_bounds__(TPB) void dists_fold_kernel(const double* __restrict__ part, int chunks, int C, int choff, int n, int HW, const float* __restrict__ feat,
                                                         RawArgs raw, double* __restrict__ mom) {
    __shared__ double s_red[TPB / 64][5];
    const int c = blockIdx.x, pair = blockIdx.y;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < chunks; i += TPB) {
        const double* q = part + (((long)pair * chunks + i) * C + c) * 5;
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j] += q[j];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            t[j] = s_red[0][j];
#pragma unroll
            for (int k = 1; k < TPB / 64; ++k) t[j] += s_red[k][j];
        }
        double ka, kb;
        if (feat) {
            ka = (double)feat[(long)pair * HW * C + c];
            kb = (double)feat[(long)(pair + n) * HW * C + c];
        } else {
            ka = (double)raw.x01[raw.a[(long)pair * raw.a_img + c]];
            kb = (double)raw.x01[raw.b[(long)pair * raw.b_img + c]];
        }
        const double N = (double)HW;
        const double dx = t[0] / N, dy = t[1] / N;
        double* q = mom + ((long)pair * IR_DISTS_CHANNELS + choff + c) * 5;
        q[0] = ka + dx;
        q[1] = kb + dy;
        q[2] = t[2] / N - dx * dx;
        q[3] = t[3] / N - dy * dy;
        q[4] = t[4] / N - dx * dy;
    }
}

// one workgroup per pair: S1, S2 and the weighted sum in fp64, the channels in a fixed order
__global__ __launch_bounds__(TPB) void dists_score_kernel(const double* __restrict__ mom, const float* __restrict__ alpha, const float* __restrict__ beta, double wsum,
                                                          double* __restrict__ out) {
    __shared__ double s_red[TPB / 64];
    const double* m = mom + (long)blockIdx.x * IR_DISTS_CHANNELS * 5;
    double sum = 0.0;
    for (int c = threadIdx.x; c < IR_DISTS_CHANNELS; c += TPB) {
        const double mx = m[5 * c], my = m[5 * c + 1], vx = m[5 * c + 2], vy = m[5 * c + 3], cxy = m[5 * c + 4];
        const double s1 = (2.0 * mx * my + 1e-6) / (mx * mx + my * my + 1e-6);
        const double s2 = (2.0 * cxy + 1e-6) / (vx + vy + 1e-6);
        sum += (double)alpha[c] * s1 + (double)beta[c] * s2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_red[0];
#pragma unroll
        for (int i = 1; i < TPB / 64; ++i) s += s_red[i];
        out[blockIdx.x] = 1.0 - s / wsum;
    }
}

constexpr int STAGE_CONVS[5] = {2, 2, 3, 3, 3};
constexpr int STAGE_WIDTH[5] = {64, 128, 256, 512, 512};
constexpr int MAP_WIDTH[IR_DISTS_MAPS] = {3, 64, 128, 256, 512, 512};

}  // namespace

int ir_dists_plan(int n, int h, int w, IrDistsPlan* pl) {
    if (n < 1 || n > 65535 || h < IR_DISTS_MIN_EDGE || w < IR_DISTS_MIN_EDGE) return -1;   // n: grid.z of the moment kernels, grid.y of the fold
    if ((double)2 * n * h * w > 2.0e9) return -1;   // M is an int
    int H = h, W = w;
    size_t part = 0;
    const size_t first = (size_t)64 * h * w;   // floats of a stage-1 map
    for (int k = 0; k < IR_DISTS_MAPS; ++k) {
        if (k >= 2) {
            H = (H + 1) / 2;
            W = (W + 1) / 2;
        }
        pl->mh[k] = H;
        pl->mw[k] = W;
        pl->chunks[k] = (int)(((long)H * W + MOM_PIX - 1) / MOM_PIX);
        part = std::max(part, (size_t)pl->chunks[k] * MAP_WIDTH[k]);
        if (k >= 1 && (size_t)H * W * MAP_WIDTH[k] > first) return -1;   // cannot happen from 16 x 16 on: every later map is smaller
    }
    pl->map_bytes = (2 * (size_t)n * first * sizeof(float) + 255) & ~(size_t)255;
    pl->part_bytes = ((size_t)n * part * 5 * sizeof(double) + 255) & ~(size_t)255;
    pl->mom_bytes = ((size_t)n * IR_DISTS_CHANNELS * 5 * sizeof(double) + 255) & ~(size_t)255;
    pl->total = 2 * pl->map_bytes + pl->part_bytes + pl->mom_bytes;
    return 0;
}

int ir_launch_dists(const IrDistsModel& m, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, void* ws,
                    double* out, double* moments, hipStream_t s) {
    IrDistsPlan pl;
    if (ir_dists_plan(n, h, w, &pl)) return -1;
    char* base = static_cast<char*>(ws);
    float* bufs[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + pl.map_bytes)};
    double* part = reinterpret_cast<double*>(base + 2 * pl.map_bytes);
    double* mom = moments ? moments : reinterpret_cast<double*>(base + 2 * pl.map_bytes + pl.part_bytes);
    const int imgs = 2 * n;

    RawArgs raw{a, b, a_pitch, (long)a_rows * a_pitch, b_pitch, (long)b_rows * b_pitch, m.x01, w, h * w};
    hipLaunchKernelGGL(dists_raw_moments_kernel, dim3(pl.chunks[0], 1, n), dim3(TPB), 0, s, raw, part);
    hipLaunchKernelGGL(dists_fold_kernel, dim3(3, n), dim3(TPB), 0, s, part, pl.chunks[0], 3, 0, n, h * w, (const float*)nullptr, raw, mom);

    const float* cur = nullptr;
    int which = 0, conv = 0, choff = 3, cin = 3;
    for (int k = 1; k <= 5; ++k) {
        const int H = pl.mh[k], W = pl.mw[k], C = STAGE_WIDTH[k - 1];
        if (k > 1) {
            const long total = (long)imgs * H * W * (cin / 4);
            hipLaunchKernelGGL(dists_pool_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, reinterpret_cast<const float4*>(cur),
                               reinterpret_cast<float4*>(bufs[which]), pl.mh[k - 1], pl.mw[k - 1], cin / 4, H, W, total);
            cur = bufs[which];
            which ^= 1;
        }
        for (int j = 0; j < STAGE_CONVS[k - 1]; ++j, ++conv) {
            ConvArgs p{};
            p.a = a; p.b = b; p.a_pitch = a_pitch; p.a_img = (long)a_rows * a_pitch; p.b_pitch = b_pitch; p.b_img = (long)b_rows * b_pitch; p.n = n;
            p.tab = m.tab; p.in = cur; p.H = H; p.W = W; p.cin = cin;
            p.M = imgs * H * W; p.K = 9 * cin; p.N = C;
            p.wgt = m.w[conv]; p.bias = m.b[conv]; p.out = bufs[which];
            const unsigned gm = (unsigned)((p.M + BM - 1) / BM);
            if (conv == 0)
                hipLaunchKernelGGL((dists_conv_kernel<64, true>), dim3(gm, C / 64), dim3(TPB), 0, s, p);
            else if (C % 128 == 0)
                hipLaunchKernelGGL((dists_conv_kernel<128, false>), dim3(gm, C / 128), dim3(TPB), 0, s, p);
            else
                hipLaunchKernelGGL((dists_conv_kernel<64, false>), dim3(gm, C / 64), dim3(TPB), 0, s, p);
            cur = bufs[which];
            which ^= 1;
            cin = C;
        }
        hipLaunchKernelGGL(dists_moments_kernel, dim3(pl.chunks[k], C / 64, n), dim3(TPB), 0, s, cur, n, H * W, C, part);
        hipLaunchKernelGGL(dists_fold_kernel, dim3(C, n), dim3(TPB), 0, s, part, pl.chunks[k], C, choff, n, H * W, cur, raw, mom);
        choff += C;
    }
    hipLaunchKernelGGL(dists_score_kernel, dim3(n), dim3(TPB), 0, s, mom, m.alpha, m.beta, m.wsum, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
