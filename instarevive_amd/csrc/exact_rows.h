// The fp64-statistics row kernels of the two transformers (musiq.hip, maniqa.hip): LayerNorm, softmax rows and the exact GELU, a wave per row,
// every sum a per-lane sequential chain followed by a fixed butterfly - no floating-point atomics, the same bits on every call.
// ONLY FOR FILES BUILT WITH -ffp-contract=off (see build.py): the products and sums here are separate operations, and a file built with
// -ffp-contract=fast would fuse them and change the bits. The kernels are static: each including file gets its own copy under its own flags.
#pragma once
#include <math.h>

#include "common.h"

constexpr int ROWS_TPB = 256;   // four rows per workgroup

IR_DEVINL double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// LayerNorm of row blockIdx.x * 4 + wave: lane l sums columns l, l + 64, ... in order, the lanes fold in a fixed butterfly
static __global__ __launch_bounds__(ROWS_TPB) void exact_ln_kernel(const float* __restrict__ x, long rows, int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   double eps, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ROWS_TPB / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;   // uniform over the wave
    const float* q = x + row * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)q[c];
    const double mean = wave_sum_d(s) / (double)C;
    double v = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)q[c] - mean;
        v += d * d;
    }
    const double rstd = 1.0 / sqrt(wave_sum_d(v) / (double)C + eps);
    for (int c = lane; c < C; c += 64) out[row * C + c] = (float)(((double)q[c] - mean) * rstd * (double)gamma[c] + (double)beta[c]);
}

// softmax of row blockIdx.x * 4 + wave of [rows][Tpad], in place over its first T columns; the columns behind them become 0
static __global__ __launch_bounds__(ROWS_TPB) void exact_softmax_kernel(float* __restrict__ s, long rows, int T, int Tpad) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ROWS_TPB / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;   // uniform over the wave
    float* q = s + row * Tpad;
    float mx = -INFINITY;
    for (int t = lane; t < T; t += 64) mx = fmaxf(mx, q[t]);
    mx = wave_max(mx);
    double sum = 0.0;
    for (int t = lane; t < T; t += 64) sum += exp((double)q[t] - (double)mx);
    sum = wave_sum_d(sum);
    for (int t = lane; t < Tpad; t += 64) q[t] = t < T ? (float)(exp((double)q[t] - (double)mx) / sum) : 0.f;
}

// the exact GELU, in place
static __global__ __launch_bounds__(ROWS_TPB) void exact_gelu_kernel(float* __restrict__ x, long total) {
    const long i = (long)blockIdx.x * ROWS_TPB + threadIdx.x;
    if (i >= total) return;
    const double v = (double)x[i];
    x[i] = (float)(0.5 * v * (1.0 + erf(v * 0.70710678118654752440)));
}

static inline unsigned blocks_of(long total, int per) { return (unsigned)((total + per - 1) / per); }

static inline void launch_ln(const float* x, long rows, int C, const float* g, const float* b, double eps, float* out, hipStream_t s) {
    hipLaunchKernelGGL(exact_ln_kernel, dim3(blocks_of(rows, ROWS_TPB / 64)), dim3(ROWS_TPB), 0, s, x, rows, C, g, b, eps, out);
}
static inline void launch_softmax(float* x, long rows, int T, int Tpad, hipStream_t s) {
    hipLaunchKernelGGL(exact_softmax_kernel, dim3(blocks_of(rows, ROWS_TPB / 64)), dim3(ROWS_TPB), 0, s, x, rows, T, Tpad);
}
static inline void launch_gelu(float* x, long total, hipStream_t s) {
    hipLaunchKernelGGL(exact_gelu_kernel, dim3(blocks_of(total, ROWS_TPB)), dim3(ROWS_TPB), 0, s, x, total);
}
