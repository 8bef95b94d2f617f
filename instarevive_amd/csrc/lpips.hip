// LPIPS v0.1 / alex of uint8 HWC RGB device images (ir_lpips): the model of tools/evaluate_pairs.py::LPIPS in exact fp32.
// The 2n images of a call (a's n, then b's n) go through one set of launches:
//   conv1 .. conv5 as implicit GEMMs on the exact-fp32 tile loop of exact_f32_tile.h, bias + ReLU in the epilogue, feature maps NHWC fp32.
//   M = output pixels of 2n images, N = cout, K = k * k * cin in (ky, kx, c) order - the weights are repacked to [K padded to 32][cout] by
//   ir_lpips_configure, zero rows behind K (363 -> 384 for conv1; the A tile is zero there as well). The tile is 128 x BN, BN = 128 where cout
//   is a multiple of 128, else 64. conv1 gathers straight from the bytes through the 3 x 256 scaling table (the host's fp32
//   ((2 (v / 255) - 1) - shift) / scale, so the network's input is the host model's to the bit); padding is 0 in that scaled domain.
//   max-pool 3 / 2 (floor mode) is a kernel of its own in front of conv2 and conv3.
//   One distance kernel per stage: a wave per pixel, channel norms and the lin-weighted squared difference of the unit vectors in fp64
//   (x / (sqrt(sum x^2) + 1e-10): an all-zero vector gives exactly 0), a fixed number of pixels per workgroup, the workgroup's sum to the
//   workspace; the last launch folds the partials of a pair stage by stage in a fixed order, divides by the stage's pixel count and adds
//   the five: a pair gives the same bits on every call and at every place in a batch.
// Reads are clipped to the compared rectangle h x w of either image; every store is guarded by the row count M of its launch.
#include <algorithm>

#include "common.h"
#include "exact_f32_tile.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int BM = 128;
constexpr int DIST_PIX = 64;   // pixels per workgroup of the distance kernel (16 per wave): the unit of the partial sums

struct ConvArgs {
    // input: the byte images (conv1) or an NHWC fp32 map
    const uint8_t *a, *b;
    long a_pitch, a_img, b_pitch, b_img;
    int n;                      // images of a (the following n are b's)
    const float* tab;           // [3][256] scaling table
    const float* in;            // [imgs][H][W][cin]
    int H, W, cin;              // input size (conv1: the byte image's h, w)
    int Ho, Wo, ks, pad;
    int M, K, N;                // M = imgs * Ho * Wo, K = ks * ks * cin (un-padded), N = cout
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

// FIRST: conv1 (stride 4, bytes through the table); else stride 1 from an fp32 map whose cin is a multiple of BK
template <int BN, bool FIRST>
__global__ __launch_bounds__(TPB, FIRST ? 2 : BN == 128 ? 3 : 4) void lpips_conv_kernel(ConvArgs p) {
    const KnB<BN, false> b{.b = p.wgt, .ldb = p.N};
    if constexpr (FIRST) {
        __shared__ float s_tab[3 * 256];
        const ByteTableA<BM, true> a{.a = p.a, .b = p.b, .a_pitch = p.a_pitch, .a_img = p.a_img, .b_pitch = p.b_pitch, .b_img = p.b_img, .n = p.n, .tab = p.tab, .s_tab = s_tab,
                                     .H = p.H, .W = p.W, .Ho = p.Ho, .Wo = p.Wo, .row_k = 33, .stride = 4, .pad = p.pad, .M = p.M, .K = p.K};   // 33 = 11 taps x 3 channels of one image row
        tile_loop<BM, BN>(a, b, p.M, p.K, BiasRelu{p});
    } else {
        const NhwcA<BM, true> a{.in = p.in, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.cin, .kw = p.ks, .stride = 1, .ph = p.pad, .pw = p.pad, .Ho = p.Ho, .Wo = p.Wo, .M = p.M, .K = p.K};
        tile_loop<BM, BN>(a, b, p.M, p.K, BiasRelu{p});
    }
}

// MaxPool2d(3, 2), floor mode: Ho = (H - 3) / 2 + 1, every window inside the map
__global__ __launch_bounds__(TPB) void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, int Ho, int Wo, long total) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const long img = r / Ho;
    const float* q = in + ((img * H + 2 * oy) * W + 2 * ox) * C + c;
    float v = q[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, q[((long)dy * W + dx) * C]);
    out[i] = v;
}

// feat: [2n][HW][C]; workgroup (x, y): pixels DIST_PIX * x .. of pair y; part[y * part_stride + x] = the sum of their distances
template <int CPL>   // channels per lane: C <= 64 * CPL
__global__ __launch_bounds__(TPB) void lpips_dist_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int n, int HW, int C, double* __restrict__ part,
                                                         int part_stride) {
    __shared__ double s_red[TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pair = blockIdx.y;
    const float* fa = feat + (long)pair * HW * C;
    const float* fb = feat + (long)(pair + n) * HW * C;
    double w[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) w[j] = lane + 64 * j < C ? (double)lin[lane + 64 * j] : 0.0;
    double sum = 0.0;
    for (int i = 0; i < DIST_PIX / (TPB / 64); ++i) {
        const int pix = blockIdx.x * DIST_PIX + i * (TPB / 64) + wave;
        if (pix >= HW) break;   // uniform over the wave
        double xa[CPL], xb[CPL], sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            xa[j] = c < C ? (double)fa[(long)pix * C + c] : 0.0;
            xb[j] = c < C ? (double)fb[(long)pix * C + c] : 0.0;
            sa += xa[j] * xa[j];
            sb += xb[j] * xb[j];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sa += __shfl_xor(sa, o);
            sb += __shfl_xor(sb, o);
        }
        const double ra = sqrt(sa) + 1e-10, rb = sqrt(sb) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const double t = xa[j] / ra - xb[j] / rb;
            d += w[j] * (t * t);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
        sum += d;
    }
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_red[0];
#pragma unroll
        for (int i = 1; i < TPB / 64; ++i) s += s_red[i];
        part[(long)pair * part_stride + blockIdx.x] = s;
    }
}

struct FoldArgs {
    int first[5], count[5];
    double pixels[5];
};

__global__ __launch_bounds__(TPB) void lpips_fold_kernel(const double* __restrict__ part, int part_stride, FoldArgs f, double* __restrict__ out) {
    __shared__ double s_red[TPB / 64];
    const double* q = part + (long)blockIdx.x * part_stride;
    double total = 0.0;
    for (int k = 0; k < 5; ++k) {
        double v = 0.0;
        for (int i = threadIdx.x; i < f.count[k]; i += TPB) v += q[f.first[k] + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        __syncthreads();   // s_red may still be read from the previous stage
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
        __syncthreads();
        double s = s_red[0];
#pragma unroll
        for (int i = 1; i < TPB / 64; ++i) s += s_red[i];
        total += s / f.pixels[k];
    }
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

struct StageShape { int cin, cout, ks, stride, pad, pool; };
constexpr StageShape STAGES[5] = {{3, 64, 11, 4, 2, 0}, {64, 192, 5, 1, 2, 1}, {192, 384, 3, 1, 1, 1}, {384, 256, 3, 1, 1, 0}, {256, 256, 3, 1, 1, 0}};

}  // namespace

int ir_lpips_plan(int n, int h, int w, IrLpipsPlan* pl) {
    if (n < 1 || h < 31 || w < 31) return -1;
    int H = h, W = w;
    size_t x = 0, y = 0;   // floats of the two ping-pong maps per image
    long chunks = 0;
    for (int k = 0; k < 5; ++k) {
        const StageShape& s = STAGES[k];
        if (s.pool) {
            H = (H - 3) / 2 + 1;
            W = (W - 3) / 2 + 1;
            pl->ph[k] = H;
            pl->pw[k] = W;
            y = std::max(y, (size_t)H * W * s.cin);
        }
        H = (H + 2 * s.pad - s.ks) / s.stride + 1;
        W = (W + 2 * s.pad - s.ks) / s.stride + 1;
        if (H < 1 || W < 1) return -1;
        pl->oh[k] = H;
        pl->ow[k] = W;
        // conv1 -> X, pool1 -> Y, conv2 -> X, pool2 -> Y, conv3 -> X, conv4 -> Y, conv5 -> X
        (k == 3 ? y : x) = std::max(k == 3 ? y : x, (size_t)H * W * s.cout);
        if ((double)2 * n * H * W > 2.0e9) return -1;   // M is an int
        pl->first[k] = (int)chunks;
        pl->count[k] = (int)(((long)H * W + DIST_PIX - 1) / DIST_PIX);
        chunks += pl->count[k];
        if (chunks > 0x7fffffffL) return -1;
    }
    if (n > 65535) return -1;   // grid.y of the distance kernel
    pl->chunks = (int)chunks;
    pl->x_bytes = (2 * (size_t)n * x * sizeof(float) + 255) & ~(size_t)255;
    pl->y_bytes = (2 * (size_t)n * y * sizeof(float) + 255) & ~(size_t)255;
    pl->part_bytes = ((size_t)n * chunks * sizeof(double) + 255) & ~(size_t)255;
    pl->total = pl->x_bytes + pl->y_bytes + pl->part_bytes;
    return 0;
}

int ir_launch_lpips(const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, const float* tab,
                    const float* const* wgt, const float* const* bias, const float* const* lin, void* ws, double* out, hipStream_t s) {
    IrLpipsPlan pl;
    if (ir_lpips_plan(n, h, w, &pl)) return -1;
    float* X = reinterpret_cast<float*>(ws);
    float* Y = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.x_bytes);
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + pl.x_bytes + pl.y_bytes);
    const int imgs = 2 * n;
    const float* cur = nullptr;
    int H = h, W = w;
    for (int k = 0; k < 5; ++k) {
        const StageShape& st = STAGES[k];
        if (st.pool) {
            const long total = (long)imgs * pl.ph[k] * pl.pw[k] * st.cin;
            hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, cur, Y, H, W, st.cin, pl.ph[k], pl.pw[k], total);
            cur = Y;
            H = pl.ph[k];
            W = pl.pw[k];
        }
        float* dst = k == 3 ? Y : X;
        ConvArgs p{};
        p.a = a; p.b = b; p.a_pitch = a_pitch; p.a_img = (long)a_rows * a_pitch; p.b_pitch = b_pitch; p.b_img = (long)b_rows * b_pitch; p.n = n;
        p.tab = tab; p.in = cur; p.H = H; p.W = W; p.cin = st.cin;
        p.Ho = pl.oh[k]; p.Wo = pl.ow[k]; p.ks = st.ks; p.pad = st.pad;
        p.M = imgs * pl.oh[k] * pl.ow[k]; p.K = st.ks * st.ks * st.cin; p.N = st.cout;
        p.wgt = wgt[k]; p.bias = bias[k]; p.out = dst;
        const unsigned gm = (unsigned)((p.M + BM - 1) / BM);
        if (k == 0)
            hipLaunchKernelGGL((lpips_conv_kernel<64, true>), dim3(gm, st.cout / 64), dim3(TPB), 0, s, p);
        else if (st.cout % 128 == 0)
            hipLaunchKernelGGL((lpips_conv_kernel<128, false>), dim3(gm, st.cout / 128), dim3(TPB), 0, s, p);
        else
            hipLaunchKernelGGL((lpips_conv_kernel<64, false>), dim3(gm, st.cout / 64), dim3(TPB), 0, s, p);
        cur = dst;
        H = pl.oh[k];
        W = pl.ow[k];
        const int HW = H * W;
        const dim3 gd(pl.count[k], n);
        double* pk = part + pl.first[k];
        if (st.cout <= 64)
            hipLaunchKernelGGL(lpips_dist_kernel<1>, gd, dim3(TPB), 0, s, cur, lin[k], n, HW, st.cout, pk, pl.chunks);
        else if (st.cout <= 256)
            hipLaunchKernelGGL(lpips_dist_kernel<4>, gd, dim3(TPB), 0, s, cur, lin[k], n, HW, st.cout, pk, pl.chunks);
        else
            hipLaunchKernelGGL(lpips_dist_kernel<6>, gd, dim3(TPB), 0, s, cur, lin[k], n, HW, st.cout, pk, pl.chunks);
    }
    FoldArgs f;
    for (int k = 0; k < 5; ++k) {
        f.first[k] = pl.first[k];
        f.count[k] = pl.count[k];
        f.pixels[k] = (double)pl.oh[k] * (double)pl.ow[k];
    }
    hipLaunchKernelGGL(lpips_fold_kernel, dim3(n), dim3(TPB), 0, s, part, pl.chunks, f, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
