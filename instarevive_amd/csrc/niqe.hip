// The pixel work of NIQE on uint8 HWC RGB device images (ir_niqe_stats): the definition of tools/evaluate_niqe.py, every operation in fp64 and in
// the model's order. Only the top-left (h / 96 * 96) x (w / 96 * 96) rectangle H x W of an image is read. Three launches, each with one
// workgroup per 96 x 96 block of the image:
//   half    the block's luma - y = rint(((t_r[r] + t_g[g]) + t_b[b]) * 255) with t_c[v] = coef_c * (double)((float)v / 255.0f) from the host's
//           tables, an integer 0 .. 255 kept as a byte in LDS with the 3-pixel halo of the 8-tap filter (symmetric padding at the rectangle's
//           edges) - then MATLAB's antialiased bicubic imresize(., 0.5) of y / 255 (a fourth table): weights (-3, -9, 29, 111, 111, 29, -9, -3)
//           / 256 over inputs 2o - 3 .. 2o + 4, down the columns first (h -> h / 2), then along the rows, each pass summed from 0.0 over taps
//           0 .. 7; times 255 into the fp64 half-size plane in the workspace.
//   stats<1> luma of the block with the 3-pixel halo of the 7 x 7 window (replicate padding at the rectangle's edges) as bytes in LDS; mu and m2
//           as 49-tap sums from 0.0 in row-major tap order, sigma = sqrt(|m2 - mu mu|), the MSCN value (y - mu) / (sigma + 1) of all 96 x 96
//           pixels into LDS (fp64, 73.7 KB); then the five fields - the value itself and its products with the neighbours (0,1), (1,0), (1,1),
//           (1,-1) taken circularly INSIDE the block - and of each the six numbers count(p < 0), count(p > 0), sum p^2 over either side,
//           sum |p|, sum p^2.
//   stats<2> the same on 48 x 48 blocks of the half-size plane.
// Every thread adds its pixels in a fixed order and the workgroup folds the thirty values in a fixed order (xor tree inside a wave, then the
// waves in turn); a block belongs to one workgroup, so there are no partial sums across workgroups and no floating-point atomics: an image
// gives the same bits on every call and at every position of a batch. Contraction into fused multiply-adds is off for the whole file - on a
// flat area y - mu is rounding noise whose SIGN decides the side of the asymmetric fit a pixel counts on, so the order of operations is part
// of the definition. The pragma below is not enough under the library's -ffp-contract=fast, which fuses in the backend whatever a pragma says:
// build.py compiles this file with -ffp-contract=off.
#include <cmath>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 512;
constexpr int WAVES = TPB / 64;
constexpr int KW = 7, R = 3;          // the MSCN window and its radius
constexpr int B1 = IR_NIQE_BLOCK;     // 96
constexpr int B2 = B1 / 2;
constexpr int HT = 8;                 // taps of the half-size filter: inputs 2o - 3 .. 2o + 4
constexpr int IN = B1 + 6;            // a block's input rows / columns of either halo (3 on each side)
constexpr int INP = (IN + 3) & ~3;    // LDS row of luma bytes

struct Window { double k[KW * KW]; };

struct Image {
    const uint8_t* p;
    long pitch, img;
    int H, W;   // the scored rectangle (multiples of 96)
};

// sum over the workgroup, valid on thread 0; the order is fixed (xor tree inside a wave, then wave 0, 1, ...)
IR_DEVINL double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) s += red[i];
    return s;
}

IR_DEVINL int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

IR_DEVINL uint8_t luma_at(const Image& im, const uint8_t* base, int gy, int gx, const double* s_tab) {
    const uint8_t* q = base + (long)gy * im.pitch + 3L * gx;
    const double y = rint(((s_tab[q[0]] + s_tab[256 + q[1]]) + s_tab[512 + q[2]]) * 255.0);   // half to even
    return (uint8_t)fmin(fmax(y, 0.0), 255.0);
}

// ---------------------------------------------------------------- the half-size plane
__global__ __launch_bounds__(TPB) void niqe_half_kernel(Image im, const double* __restrict__ tab, double* __restrict__ half) {
    __shared__ double s_tab[4 * 256];
    __shared__ uint8_t s_y[IN][INP];
    __shared__ double s_v[B2][IN];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * B1, y0 = blockIdx.y * B1, image = blockIdx.z;
    for (int i = tid; i < 4 * 256; i += TPB) s_tab[i] = tab[i];
    __syncthreads();
    const uint8_t* base = im.p + (long)image * im.img;
    for (int i = tid; i < IN * IN; i += TPB) {
        const int ly = i / IN, lx = i - ly * IN;
        int gy = y0 - R + ly, gx = x0 - R + lx;
        gy = gy < 0 ? -gy - 1 : (gy >= im.H ? 2 * im.H - 1 - gy : gy);   // symmetric: -1 -> 0, H -> H - 1
        gx = gx < 0 ? -gx - 1 : (gx >= im.W ? 2 * im.W - 1 - gx : gx);
        s_y[ly][lx] = luma_at(im, base, clampi(gy, 0, im.H - 1), clampi(gx, 0, im.W - 1), s_tab);
    }
    __syncthreads();
    const double wt[HT] = {-3.0 / 256, -9.0 / 256, 29.0 / 256, 111.0 / 256, 111.0 / 256, 29.0 / 256, -9.0 / 256, -3.0 / 256};
    const double* unit = s_tab + 768;   // y / 255.0
    for (int i = tid; i < B2 * IN; i += TPB) {   // down the columns: output row oy of input column lx
        const int oy = i / IN, lx = i - oy * IN;
        double a = 0.0;
#pragma unroll
        for (int t = 0; t < HT; ++t) a += wt[t] * unit[s_y[2 * oy + t][lx]];
        s_v[oy][lx] = a;
    }
    __syncthreads();
    const int H2 = im.H / 2, W2 = im.W / 2;
    double* out = half + (long)image * H2 * W2 + (long)(blockIdx.y * B2) * W2 + blockIdx.x * B2;
    for (int i = tid; i < B2 * B2; i += TPB) {
        const int oy = i / B2, ox = i - oy * B2;
        double a = 0.0;
#pragma unroll
        for (int t = 0; t < HT; ++t) a += wt[t] * s_v[oy][2 * ox + t];
        out[(long)oy * W2 + ox] = a * 255.0;
    }
}

// ---------------------------------------------------------------- MSCN and the thirty sums of a block
// dynamic LDS: the MSCN block [B][B] doubles, the reduction scratch, then either the luma tables and the luma bytes (scale 1) or the block's
// half-size values with their halo as doubles (scale 2)
template <int SCALE>
constexpr size_t stats_lds() {
    constexpr int B = B1 / SCALE;
    return (size_t)(B * B + WAVES) * 8 + (SCALE == 1 ? (size_t)768 * 8 + (size_t)IN * INP : (size_t)(B + 2 * R) * (B + 2 * R) * 8);
}

template <int SCALE>
__global__ __launch_bounds__(TPB) void niqe_stats_kernel(Image im, const double* __restrict__ tab, const double* __restrict__ half, Window win,
                                                         double* __restrict__ out) {
    constexpr int B = B1 / SCALE, I = B + 2 * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char niqe_smem[];
    double* s_m = reinterpret_cast<double*>(niqe_smem);   // [B][B]
    double* s_red = s_m + B * B;
    double* s_tab = s_red + WAVES;                        // scale 1: [3][256]
    uint8_t* s_yb = reinterpret_cast<uint8_t*>(s_tab + 768);   // scale 1: [I][INP]
    double* s_yd = s_red + WAVES;                         // scale 2: [I][I]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * B, y0 = blockIdx.y * B, image = blockIdx.z;
    const int H = im.H / SCALE, W = im.W / SCALE;

    // the block's values with the window's halo, replicate padding at the rectangle's edges
    if constexpr (SCALE == 1) {
        for (int i = tid; i < 768; i += TPB) s_tab[i] = tab[i];
        __syncthreads();
        const uint8_t* base = im.p + (long)image * im.img;
        for (int i = tid; i < I * I; i += TPB) {
            const int ly = i / I, lx = i - ly * I;
            s_yb[ly * INP + lx] = luma_at(im, base, clampi(y0 - R + ly, 0, H - 1), clampi(x0 - R + lx, 0, W - 1), s_tab);
        }
    } else {
        const double* src = half + (long)image * H * W;
        for (int i = tid; i < I * I; i += TPB) {
            const int ly = i / I, lx = i - ly * I;
            s_yd[ly * I + lx] = src[(long)clampi(y0 - R + ly, 0, H - 1) * W + clampi(x0 - R + lx, 0, W - 1)];
        }
    }
    __syncthreads();

    for (int i = tid; i < B * B; i += TPB) {
        const int py = i / B, px = i - py * B;
        double mu = 0.0, m2 = 0.0;
#pragma unroll
        for (int a = 0; a < KW; ++a)
#pragma unroll
            for (int b = 0; b < KW; ++b) {
                double y;
                if constexpr (SCALE == 1) y = (double)s_yb[(py + a) * INP + px + b];
                else y = s_yd[(py + a) * I + px + b];
                const double k = win.k[a * KW + b];
                mu += k * y;
                m2 += k * (y * y);
            }
        double yc;
        if constexpr (SCALE == 1) yc = (double)s_yb[(py + R) * INP + px + R];
        else yc = s_yd[(py + R) * I + px + R];
        const double sigma = sqrt(fabs(m2 - mu * mu));
        s_m[i] = (yc - mu) / (sigma + 1.0);
    }
    __syncthreads();

    // [field][count <0, count >0, sum p^2 <0, sum p^2 >0, sum |p|, sum p^2]; the counts are exact in fp64 (at most 9216)
    double acc[5][6];
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[f][k] = 0.0;
    for (int i = tid; i < B * B; i += TPB) {
        const int py = i / B, px = i - py * B;
        const int pu = py == 0 ? B - 1 : py - 1, pl = px == 0 ? B - 1 : px - 1, pr = px == B - 1 ? 0 : px + 1;
        const double m = s_m[i];
        const double p[5] = {m, m * s_m[py * B + pl], m * s_m[pu * B + px], m * s_m[pu * B + pl], m * s_m[pu * B + pr]};
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            const double v = p[f], sq = v * v;
            if (v < 0.0) {
                acc[f][0] += 1.0;
                acc[f][2] += sq;
            } else if (v > 0.0) {
                acc[f][1] += 1.0;
                acc[f][3] += sq;
            }
            acc[f][4] += fabs(v);
            acc[f][5] += sq;
        }
    }
    const long blocks = (long)gridDim.x * gridDim.y;
    double* o = out + ((((long)image * 2 + (SCALE - 1)) * blocks) + (long)blockIdx.y * gridDim.x + blockIdx.x) * 30;
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double t = block_sum(acc[f][k], s_red);
            if (tid == 0) o[f * 6 + k] = t;
        }
}

}  // namespace

void ir_niqe_window_host(double* k49) {
    // exp(-(i^2 + j^2) / (2 sigma^2)), sigma = 7 / 6, entries below eps * max zeroed, divided by the sum (MATLAB's fspecial('gaussian'))
    const double sigma = 7.0 / 6.0;
    double mx = 0.0, sum = 0.0;
    for (int a = 0; a < KW; ++a)
        for (int b = 0; b < KW; ++b) {
            const double i = a - R, j = b - R;
            const double v = std::exp(-(i * i + j * j) / (2.0 * sigma * sigma));
            k49[a * KW + b] = v;
            mx = v > mx ? v : mx;
        }
    for (int t = 0; t < KW * KW; ++t) {
        if (k49[t] < 2.220446049250313e-16 * mx) k49[t] = 0.0;
        sum += k49[t];
    }
    for (int t = 0; t < KW * KW; ++t) k49[t] /= sum;
}

int ir_launch_niqe_stats(const uint8_t* img, int rows, long pitch, int n, int h, int w, const double* tab, double* half, double* out, hipStream_t s) {
    const int by = h / B1, bx = w / B1;
    if (by < 1 || bx < 1 || n < 1 || n > 65535 || by > 65535) return -1;   // grid.y / grid.z
    static_assert(stats_lds<1>() <= 160 * 1024 && stats_lds<2>() <= 64 * 1024, "a block's MSCN values and luma must fit in LDS");
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(niqe_stats_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stats_lds<1>()) != hipSuccess)
        return -1;
    Window win;
    ir_niqe_window_host(win.k);
    Image im{img, pitch, (long)rows * pitch, by * B1, bx * B1};
    const dim3 grid(bx, by, n);
    hipLaunchKernelGGL(niqe_half_kernel, grid, dim3(TPB), 0, s, im, tab, half);
    hipLaunchKernelGGL(niqe_stats_kernel<1>, grid, dim3(TPB), stats_lds<1>(), s, im, tab, half, win, out);
    hipLaunchKernelGGL(niqe_stats_kernel<2>, grid, dim3(TPB), stats_lds<2>(), s, im, tab, half, win, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
