// LPIPS v0.1 / alex of uint8 HWC RGB device images (ir_lpips): the model of tools/evaluate_pairs.py::LPIPS in exact fp32.
// The 2n images of a call (a's n, then b's n) go through one set of launches:
//   conv1 .. conv5 as implicit GEMMs on the fp32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, so an output
//   element does not depend on the tile it falls in), bias + ReLU in the epilogue, feature maps NHWC fp32. M = output pixels of 2n images,
//   N = cout, K = k * k * cin in (ky, kx, c) order - the weights are repacked to [K padded to 32][cout] by ir_lpips_configure, zero rows
//   behind K (363 -> 384 for conv1; the A tile is zero there as well). A workgroup of four waves owns a 128 x BN tile (BN = 128 where cout
//   is a multiple of 128, else 64), a wave 64 x BN / 2 as 32 x 32 blocks; the 32-deep k-tile goes global -> registers -> LDS with the next
//   tile's loads in flight during the MFMAs. conv1 gathers straight from the bytes through the 3 x 256 scaling table (the host's fp32
//   ((2 (v / 255) - 1) - shift) / scale, so the network's input is the host model's to the bit); padding is 0 in that scaled domain.
//   max-pool 3 / 2 (floor mode) is a kernel of its own in front of conv2 and conv3.
//   One distance kernel per stage: a wave per pixel, channel norms and the lin-weighted squared difference of the unit vectors in fp64
//   (x / (sqrt(sum x^2) + 1e-10): an all-zero vector gives exactly 0), a fixed number of pixels per workgroup, the workgroup's sum to the
//   workspace; the last launch folds the partials of a pair stage by stage in a fixed order, divides by the stage's pixel count and adds
//   the five. No floating-point atomics: a pair gives the same bits on every call and at every place in a batch.
// Reads are clipped to the compared rectangle h x w of either image; every store is guarded by the row count M of its launch.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int TPB = 256;
constexpr int BM = 128, BK = 32;
constexpr int LDA = BM + 4;
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

// FIRST: conv1 (stride 4, bytes through the table); else stride 1 from an fp32 map whose cin is a multiple of BK
template <int BN, bool FIRST>
__global__ __launch_bounds__(TPB) void lpips_conv_kernel(ConvArgs p) {
    constexpr int TN = BN / 64;           // 32-column blocks per wave
    constexpr int LDB = BN + 4;
    constexpr int BV = BK * BN / 4 / TPB; // float4 of the weight tile per thread
    __shared__ float s_a[BK][LDA];
    __shared__ float s_b[BK][LDB];
    __shared__ float s_tab[FIRST ? 3 * 256 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int HWo = p.Ho * p.Wo;
    const int nk = (p.K + BK - 1) / BK;

    // the rows this thread gathers
    constexpr int AR = FIRST ? BM * BK / TPB : BM * BK / 4 / TPB;   // 16 scalars of one k / 4 float4
    const uint8_t* rb[FIRST ? AR : 1];
    long ro[FIRST ? 1 : AR];
    int riy[AR], rix[AR];
    bool rsec[FIRST ? AR : 1];   // conv1: the row belongs to an image of b (its pitch)
    if constexpr (FIRST) {
        for (int i = tid; i < 3 * 256; i += TPB) s_tab[i] = p.tab[i];
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + (tid >> 5) + 8 * i;
            if (m < p.M) {
                const int img = m / HWo, r = m - img * HWo, oy = r / p.Wo, ox = r - oy * p.Wo;
                riy[i] = oy * 4 - p.pad;
                rix[i] = ox * 4 - p.pad;
                rb[i] = img < p.n ? p.a + (long)img * p.a_img : p.b + (long)(img - p.n) * p.b_img;
                rb[i] += (long)riy[i] * (img < p.n ? p.a_pitch : p.b_pitch) + 3L * rix[i];
                rsec[i] = img >= p.n;
            } else {
                riy[i] = -(1 << 20);   // every tap out of bounds
                rix[i] = 0;
                rb[i] = p.a;
                rsec[i] = false;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + (tid >> 3) + 32 * i;
            if (m < p.M) {
                const int img = m / HWo, r = m - img * HWo, oy = r / p.Wo, ox = r - oy * p.Wo;
                riy[i] = oy - p.pad;
                rix[i] = ox - p.pad;
                ro[i] = (((long)img * p.H + riy[i]) * p.W + rix[i]) * p.cin;
            } else {
                riy[i] = -(1 << 20);
                rix[i] = 0;
                ro[i] = 0;
            }
        }
    }

    float ga[FIRST ? AR : 1];
    float4 gv[FIRST ? 1 : AR];
    float4 gb[BV];
    auto load_tile = [&](int kt) {
        const int k0 = kt * BK;
        if constexpr (FIRST) {
            const int k = k0 + (tid & 31);
            const int ky = k / 33, r = k - ky * 33, kx = r / 3, c = r - kx * 3;   // 33 = 11 taps x 3 channels of one image row
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int iy = riy[i] + ky, ix = rix[i] + kx;
                float v = 0.f;
                if (k < p.K && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
                    const uint8_t byte = rb[i][(long)ky * (rsec[i] ? p.b_pitch : p.a_pitch) + r];
                    v = s_tab[256 * c + byte];
                }
                ga[i] = v;
            }
        } else {
            const int tap = k0 / p.cin, c0 = k0 - tap * p.cin + 4 * (tid & 7);
            const int ky = tap / p.ks, kx = tap - ky * p.ks;
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int iy = riy[i] + ky, ix = rix[i] + kx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                    v = *reinterpret_cast<const float4*>(p.in + ro[i] + ((long)ky * p.W + kx) * p.cin + c0);
                gv[i] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = tid + i * TPB, kr = idx / (BN / 4), nc = idx - kr * (BN / 4);
            gb[i] = *reinterpret_cast<const float4*>(p.wgt + (long)(k0 + kr) * p.N + n0 + 4 * nc);   // rows up to Kpad exist, N is a multiple of BN
        }
    };
    auto store_tile = [&]() {
        if constexpr (FIRST) {
#pragma unroll
            for (int i = 0; i < AR; ++i) s_a[tid & 31][(tid >> 5) + 8 * i] = ga[i];
        } else {
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const int row = (tid >> 3) + 32 * i, kq = 4 * (tid & 7);
                s_a[kq][row] = gv[i].x;
                s_a[kq + 1][row] = gv[i].y;
                s_a[kq + 2][row] = gv[i].z;
                s_a[kq + 3][row] = gv[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = tid + i * TPB, kr = idx / (BN / 4), nc = idx - kr * (BN / 4);
            *reinterpret_cast<float4*>(&s_b[kr][4 * nc]) = gb[i];
        }
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if constexpr (FIRST) __syncthreads();   // the table
    load_tile(0);
    const int kh = lane >> 5, l31 = lane & 31;
    for (int kt = 0; kt < nk; ++kt) {
        store_tile();
        __syncthreads();
        if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float fa[2], fb[TN];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = s_a[kk + kh][wm * 64 + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = s_b[kk + kh][wn * (BN / 2) + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // bias + ReLU; the column is on the lane, so a row of the tile is one 128-byte store per wave
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (BN / 2) + j * 32 + l31;
        const float bias = p.bias[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 64 + i * 32 + mfma_row(r, lane);
                if (m < p.M) p.out[(long)m * p.N + col] = fmaxf(acc[i][j][r] + bias, 0.f);
            }
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
