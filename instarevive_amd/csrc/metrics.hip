// PSNR-Y / SSIM-Y of uint8 HWC RGB device images against ground truth (ir_metrics_y): the definitions of tools/evaluate_pairs.py (pyiqa's),
// every statistic in fp64. Two launches. The first: one workgroup per IR_METRICS_TH x IR_METRICS_TW tile of the SSIM map. It reads the tile's
// pixels plus the 10-pixel halo of the 11-tap window from both images, turns each into luma once - s = 16 + t_r[r] + t_g[g] + t_b[b] with
// t_k[v] = c_k * (double)((float)v / 255.0f) from the host's tables (the model divides in float32 first; the tables make the luma the
// model's to the bit) - and keeps round(s / 255 * 255) of both as bytes in LDS (16 .. 235). The pixels a tile OWNS (its own rows and
// columns; the last tile of a row / column also owns the halo up to the image's edge) add (s_a / 255 - s_b / 255)^2 to the tile's MSE sum.
// Then the horizontal pass of the five maps x, y, x^2, y^2, xy into LDS (fp64), the vertical pass and the SSIM formula per output, and a
// reduction over the workgroup (wave shuffles, then the four waves in order). Each workgroup writes its two sums to the workspace; the
// second launch, one workgroup per image, folds them in a fixed order - no floating-point atomics, so a pair gives the same bits on every
// call and at every place in a batch. Contraction into fused multiply-adds is off for the whole file: the luma follows the model's order of
// operations, and identical images give exactly 1 (2 mu1 mu2 + C1 and mu1^2 + mu2^2 + C1 round alike only as separate operations).
// Loads are clipped to the compared rectangle h x w, so nothing outside [h][3 w] of either image is read.
#include <cmath>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int TW = IR_METRICS_TW, TH = IR_METRICS_TH;
constexpr int K = 11, HALO = K - 1;
constexpr int IW = TW + HALO, IH = TH + HALO;
constexpr int IWP = (IW + 3) & ~3;   // LDS row of luma bytes

struct Window { double g[K]; };

struct Pair {
    const uint8_t *a, *b;
    long a_pitch, a_img, b_pitch, b_img;
    int h, w;
};

// sum over the workgroup, valid on thread 0; the order is fixed (xor tree inside a wave, then wave 0, 1, 2, 3)
IR_DEVINL double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < TPB / 64; ++i) s += red[i];
    return s;
}

__global__ __launch_bounds__(TPB) void metrics_tile_kernel(Pair p, const double* __restrict__ tab, Window win, double* __restrict__ part) {
    __shared__ double s_tab[3 * 256];
    __shared__ uint8_t s_ya[IH][IWP], s_yb[IH][IWP];
    __shared__ double s_h[5][IH][TW];
    __shared__ double s_red[TPB / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, image = blockIdx.z;
    for (int i = tid; i < 3 * 256; i += TPB) s_tab[i] = tab[i];
    __syncthreads();

    // luma of the tile and its halo; the squared unit-scale difference of the pixels this tile owns
    const int own_y1 = blockIdx.y == gridDim.y - 1 ? p.h : y0 + TH;
    const int own_x1 = blockIdx.x == gridDim.x - 1 ? p.w : x0 + TW;
    const uint8_t* pa = p.a + (long)image * p.a_img;
    const uint8_t* pb = p.b + (long)image * p.b_img;
    double se = 0.0;
    for (int i = tid; i < IH * IW; i += TPB) {
        const int ly = i / IW, lx = i - ly * IW;
        const int gy = y0 + ly, gx = x0 + lx;
        uint8_t ya = 0, yb = 0;
        if (gy < p.h && gx < p.w) {
            const uint8_t* qa = pa + (long)gy * p.a_pitch + 3L * gx;
            const uint8_t* qb = pb + (long)gy * p.b_pitch + 3L * gx;
            const double sa = 16.0 + s_tab[qa[0]] + s_tab[256 + qa[1]] + s_tab[512 + qa[2]];
            const double sb = 16.0 + s_tab[qb[0]] + s_tab[256 + qb[1]] + s_tab[512 + qb[2]];
            ya = (uint8_t)rint(sa / 255.0 * 255.0);   // half to even, as numpy's round
            yb = (uint8_t)rint(sb / 255.0 * 255.0);
            if (gy < own_y1 && gx < own_x1) {
                const double d = sa / 255.0 - sb / 255.0;
                se += d * d;
            }
        }
        s_ya[ly][lx] = ya;
        s_yb[ly][lx] = yb;
    }
    __syncthreads();

    // horizontal pass of x, y, x^2, y^2, xy
    for (int i = tid; i < IH * TW; i += TPB) {
        const int ly = i / TW, lx = i - ly * TW;
        double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0, f4 = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double x = (double)s_ya[ly][lx + k], y = (double)s_yb[ly][lx + k], g = win.g[k];
            f0 += g * x;
            f1 += g * y;
            f2 += g * (x * x);
            f3 += g * (y * y);
            f4 += g * (x * y);
        }
        s_h[0][ly][lx] = f0; s_h[1][ly][lx] = f1; s_h[2][ly][lx] = f2; s_h[3][ly][lx] = f3; s_h[4][ly][lx] = f4;
    }
    __syncthreads();

    // vertical pass and the SSIM map of the outputs inside the 'valid' extent
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    double ss = 0.0;
    for (int i = tid; i < TH * TW; i += TPB) {
        const int oy = i / TW, ox = i - oy * TW;
        if (y0 + oy < p.h - HALO && x0 + ox < p.w - HALO) {
            double m1 = 0.0, m2 = 0.0, f11 = 0.0, f22 = 0.0, f12 = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double g = win.g[k];
                m1 += g * s_h[0][oy + k][ox];
                m2 += g * s_h[1][oy + k][ox];
                f11 += g * s_h[2][oy + k][ox];
                f22 += g * s_h[3][oy + k][ox];
                f12 += g * s_h[4][oy + k][ox];
            }
            const double s11 = f11 - m1 * m1, s22 = f22 - m2 * m2, s12 = f12 - m1 * m2;
            const double cs = fmax((2.0 * s12 + c2) / (s11 + s22 + c2), 0.0);
            ss += (2.0 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1) * cs;
        }
    }
    const double tse = block_sum(se, s_red);
    const double tss = block_sum(ss, s_red);
    if (tid == 0) {
        double* o = part + 2 * (((long)image * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        o[0] = tse;
        o[1] = tss;
    }
}

__global__ __launch_bounds__(TPB) void metrics_fold_kernel(const double* __restrict__ part, int tiles, double pixels, double windows, double* __restrict__ out) {
    __shared__ double s_red[TPB / 64];
    const double* q = part + 2L * blockIdx.x * tiles;
    double se = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < tiles; i += TPB) {
        se += q[2 * i];
        ss += q[2 * i + 1];
    }
    const double tse = block_sum(se, s_red);
    const double tss = block_sum(ss, s_red);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = tse / pixels;
        out[2 * blockIdx.x + 1] = tss / windows;
    }
}

}  // namespace

int ir_launch_metrics_y(const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, const double* tab,
                        double* part, double* out, hipStream_t s) {
    const int tx = (w - HALO + TW - 1) / TW, ty = (h - HALO + TH - 1) / TH;
    if (tx < 1 || ty < 1 || n > 65535 || ty > 65535 || (long)tx * ty > 0x7fffffffL) return -1;   // grid.y / grid.z
    // the window of the model: exp(-c^2 / (2 sigma^2)), c = -5 .. 5, sigma 1.5, normalised to sum 1
    Window win;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double c = (double)k - (K - 1) / 2.0;
        win.g[k] = std::exp(-(c * c) / (2 * 1.5 * 1.5));
        sum += win.g[k];
    }
    for (int k = 0; k < K; ++k) win.g[k] /= sum;
    Pair p{a, b, a_pitch, (long)a_rows * a_pitch, b_pitch, (long)b_rows * b_pitch, h, w};
    hipLaunchKernelGGL(metrics_tile_kernel, dim3(tx, ty, n), dim3(TPB), 0, s, p, tab, win, part);
    hipLaunchKernelGGL(metrics_fold_kernel, dim3(n), dim3(TPB), 0, s, part, tx * ty, (double)h * (double)w, (double)(h - HALO) * (double)(w - HALO), out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
