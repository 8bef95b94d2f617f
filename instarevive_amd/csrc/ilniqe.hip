// The pixel work of IL-NIQE on uint8 HWC RGB device images (ir_ilniqe_stats; tools/evaluate_ilniqe.py is the definition, and the header states
// it): the resize to 524 x 524, the 109 planes of both scales and the 558 statistics of every block, launched per image in stream order by
// ir_launch_ilniqe_stats at the end of this file. Its two numerical building blocks are entries of their own: the dense fp64 2-D DFT of 252 or
// 504 points that carries the log-Gabor filter bank (ir_op_dft2_f64), and the Weibull maximum-likelihood fit of the magnitude planes' blocks
// (ir_op_weibull_fit). All arithmetic is fp64, nothing uses floating-point atomics and every sum has a fixed order, so an input gives the same
// bits on every call. Contraction into fused multiply-adds is off for the whole file (build.py: -ffp-contract=off, as for niqe.hip): plane 0
// and the colour planes have to equal the numpy model's bits.
//
//   dft2     Y = W X W with W[j][k] = cos(2 pi jk / N) -/+ i sin(2 pi jk / N) (forward / inverse; the inverse is scaled by 1 / N^2), as two
//            complex matrix products C[m][n] = sum_k At[k][m] B[k][n] on v_mfma_f64_16x16x4_f64. Both operands are read as P[k][index]: lane l
//            holds k = k0 + (l >> 4), index = tile + (l & 15), so sixteen lanes read 128 consecutive bytes. The first product takes At = W (W is
//            symmetric), B = X and stores its result TRANSPOSED into the workspace, so the second product (At = that, B = W) reads it the same
//            way. One wave owns a 32 x 32 tile of C (2 x 2 MFMA tiles, real and imaginary accumulators: 16 MFMAs per k step of 4, 8 when X is
//            real). 252 and 504 are multiples of 4 and not of 16: K is never padded, rows and columns beyond N are loaded as zeros and not
//            stored. The accumulator layout is the f64 one: col = lane & 15, row = (lane >> 4) + 4 * reg.
//            The real part accumulates sum Are Bre first and then sum (-Aim) Bim inside each k step, the imaginary part Are Bim then Aim Bre.
//   weibull  one workgroup per row of `count` positive values (at most IR_WEIBULL_MAX, a scale-1 block): ln x in LDS; k0 = 1.2 / std(ln x)
//            (unbiased); Newton on f(k) = S1 / S0 - mean(ln x) - 1 / k with S_j = sum x^k (ln x)^j, x^k = exp(k ln x),
//            f'(k) = S2 / S0 - (S1 / S0)^2 + 1 / k^2; at most 50 steps, stop when |k - k_prev| < 1e-2; lambda = (S0(k) / count)^(1 / k).
#include <cmath>

#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

struct DftArgs {
    const double *a_re, *a_im;   // At[k][m]
    const double *b_re, *b_im;   // B[k][n]; b_im may be null (a real operand)
    const double* b_mul;         // null, or a real plane B is multiplied by on load (the log-Gabor filter)
    double *c_re, *c_im;
    long a_zs, mul_zs, c_zs;     // doubles from one transform of the batch (blockIdx.z) to the next
    int N;
    int store_t;                 // store C[m][n] at [n][m]
    double a_sign, b_sign;       // the sign the imaginary part of At / B is read with (conjugation of W)
    double scale;
};

IR_DEVINL double ld(const double* p, int k, int idx, int N) { return idx < N ? p[(long)k * N + idx] : 0.0; }

template <bool REAL_B>
__global__ __launch_bounds__(64) void dft_gemm_kernel(DftArgs g) {
    const int lane = threadIdx.x, l15 = lane & 15, kq = lane >> 4, N = g.N;
    const int m0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const long z = blockIdx.z;
    g.a_re += z * g.a_zs;
    g.a_im += z * g.a_zs;
    if (g.b_mul) g.b_mul += z * g.mul_zs;
    g.c_re += z * g.c_zs;
    g.c_im += z * g.c_zs;
    double4_t re[2][2], im[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) re[i][j] = im[i][j] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < N; k0 += 4) {   // N % 4 == 0: k is always inside
        const int k = k0 + kq;
        double ar[2], ai[2], br[2], bi[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ar[i] = ld(g.a_re, k, m0 + 16 * i + l15, N);
            ai[i] = g.a_sign * ld(g.a_im, k, m0 + 16 * i + l15, N);
            br[i] = ld(g.b_re, k, n0 + 16 * i + l15, N);
            bi[i] = REAL_B ? 0.0 : g.b_sign * ld(g.b_im, k, n0 + 16 * i + l15, N);
            if (g.b_mul) {
                const double f = ld(g.b_mul, k, n0 + 16 * i + l15, N);
                br[i] = f * br[i];
                bi[i] = f * bi[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], re[i][j], 0, 0, 0);
                im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], br[j], im[i][j], 0, 0, 0);
                if (!REAL_B) {
                    re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai[i], bi[j], re[i][j], 0, 0, 0);
                    im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], im[i][j], 0, 0, 0);
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * i + kq + 4 * r, n = n0 + 16 * j + l15;
                if (m < N && n < N) {
                    const long at = g.store_t ? (long)n * N + m : (long)m * N + n;
                    g.c_re[at] = re[i][j][r] * g.scale;
                    g.c_im[at] = im[i][j][r] * g.scale;
                }
            }
}

// ---------------------------------------------------------------- the Weibull fit
constexpr int WTPB = 256;
constexpr int WWAVES = WTPB / 64;

// sum over the workgroup, valid on every thread; the order is fixed (xor tree inside a wave, then wave 0, 1, ...)
IR_DEVINL double wg_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // red may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int i = 1; i < WWAVES; ++i) s += red[i];
    return s;
}

// the 27 magnitude planes of IL-NIQE in the order of the statistics: planes 1-3, then 85-108
IR_DEVINL int magnitude_plane(int j) { return j < 3 ? 1 + j : 82 + j; }

// B == 0: row blockIdx.x of x [rows][count]. B > 0: block blockIdx.x (row-major, N / B per row) of magnitude plane blockIdx.y of x [109][N][N],
// count = B * B, written to the image's statistics at out[block][IR_ILNIQE_STATS] + 504 + 2 * blockIdx.y
__global__ __launch_bounds__(WTPB) void weibull_kernel(const double* __restrict__ x, int count, double* __restrict__ out, int B, int N) {
    __shared__ double s_l[IR_WEIBULL_MAX];
    __shared__ double s_red[WWAVES];
    const int tid = threadIdx.x;
    const double* row = x + (long)blockIdx.x * count;
    if (B > 0) {
        const int per = N / B;
        row = x + (long)magnitude_plane(blockIdx.y) * N * N + (long)(blockIdx.x / per) * B * N + (blockIdx.x % per) * B;
        out += (long)blockIdx.x * IR_ILNIQE_STATS + 504 + 2 * blockIdx.y - 2 * blockIdx.x;
    }
    double a = 0.0;
    for (int i = tid; i < count; i += WTPB) {
        const double l = log(B > 0 ? row[(long)(i / B) * N + i % B] : row[i]);
        s_l[i] = l;
        a += l;
    }
    const double mean = wg_sum(a, s_red) / count;
    a = 0.0;
    for (int i = tid; i < count; i += WTPB) {
        const double d = s_l[i] - mean;
        a += d * d;
    }
    double k = 1.2 / sqrt(wg_sum(a, s_red) / (count - 1));
    for (int step = 0; step < 50; ++step) {   // k and every sum are the same on all threads: the loop is uniform
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = tid; i < count; i += WTPB) {
            const double l = s_l[i], e = exp(k * l);
            s0 += e;
            s1 += e * l;
            s2 += e * (l * l);
        }
        s0 = wg_sum(s0, s_red);
        s1 = wg_sum(s1, s_red);
        s2 = wg_sum(s2, s_red);
        const double r = s1 / s0;
        const double f = r - mean - 1.0 / k, df = s2 / s0 - r * r + 1.0 / (k * k);
        const double kn = k - f / df;
        const bool done = fabs(kn - k) < 1e-2;
        k = kn;
        if (done) break;
    }
    double s0 = 0.0;
    for (int i = tid; i < count; i += WTPB) s0 += exp(k * s_l[i]);
    s0 = wg_sum(s0, s_red);
    if (tid == 0) {
        out[2 * blockIdx.x] = k;
        out[2 * blockIdx.x + 1] = pow(s0 / count, 1.0 / k);
    }
}


// ---------------------------------------------------------------- the image-level pixel work (ir_ilniqe_stats)
constexpr int NS = IR_ILNIQE_SIZE, N1 = IR_ILNIQE_USED;   // 524, 504
constexpr double IL_EPS = 1e-8, K_LOG = 1e-5;

struct Plan {   // views into the device copy of ir_ilniqe_plan's tables
    const int *idx0, *idx1;
    const double *w0, *w1;
    int P0, P1;
};
struct Win5 { double k[25]; };
struct Win6 { double k[36]; };
struct Taps { double xg[11], g[11]; };

IR_DEVINL int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// down the columns: tmp[oy][j] for the 504 used rows and the 3 w bytes of an image row
__global__ __launch_bounds__(256) void resize_cols_kernel(const uint8_t* __restrict__ img, long pitch, int w3, Plan pl, double* __restrict__ tmp) {
    const int j = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (j >= w3) return;
    double a = 0.0;
    for (int t = 0; t < pl.P0; ++t) a += pl.w0[oy * pl.P0 + t] * (double)img[(long)pl.idx0[oy * pl.P0 + t] * pitch + j];
    tmp[(long)oy * w3 + j] = a;
}

// along the rows, the clamp, and the opponent planes: rgbo [6][504][504] = R, G, B, O1, O2, O3
__global__ __launch_bounds__(256) void resize_rows_kernel(const double* __restrict__ tmp, int w3, Plan pl, double* __restrict__ rgbo) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ox >= N1) return;
    double c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double a = 0.0;
        for (int t = 0; t < pl.P1; ++t) a += pl.w1[ox * pl.P1 + t] * tmp[(long)oy * w3 + 3 * pl.idx1[ox * pl.P1 + t] + ch];
        c[ch] = fmin(fmax(a, 0.0), 255.0);
    }
    const long NN = (long)N1 * N1, at = (long)oy * N1 + ox;
    rgbo[at] = c[0];
    rgbo[NN + at] = c[1];
    rgbo[2 * NN + at] = c[2];
    rgbo[3 * NN + at] = (0.3 * c[0] + 0.04 * c[1]) - 0.35 * c[2];
    rgbo[4 * NN + at] = (0.34 * c[0] - 0.6 * c[1]) + 0.17 * c[2];
    rgbo[5 * NN + at] = (0.06 * c[0] + 0.63 * c[1]) + 0.27 * c[2];
}

// the 6 x 6 filter between the scales (correlation, replicate padding, taps -2 .. +3) at the kept positions 0, 2, 4, ...; blockIdx.z: the plane
__global__ __launch_bounds__(256) void down6_kernel(const double* __restrict__ src, double* __restrict__ dst, int N, Win6 win) {
    const int H = N / 2, x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= H) return;
    const double* s = src + (long)blockIdx.z * N * N;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) a += win.k[6 * i + j] * s[(long)clampi(2 * y - 2 + i, 0, N - 1) * N + clampi(2 * x - 2 + j, 0, N - 1)];
    dst[(long)blockIdx.z * H * H + (long)y * H + x] = a;
}

__global__ __launch_bounds__(256) void mscn_kernel(const double* __restrict__ src, double* __restrict__ dst, int N, Win5 win) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= N) return;
    double mu = 0.0, m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const double v = src[(long)clampi(y - 2 + i, 0, N - 1) * N + clampi(x - 2 + j, 0, N - 1)];
            mu += win.k[5 * i + j] * v;
            m2 += win.k[5 * i + j] * (v * v);
        }
    dst[(long)y * N + x] = (src[(long)y * N + x] - mu) / (sqrt(fabs(m2 - mu * mu)) + 1.0);
}

// log(x) of a positive normal double with IEEE additions, multiplications and one division only, in the order the definition states (the
// argument reduction and the polynomial of fdlibm's e_log.c, always in its 0.5 f^2 form): the same bits as the numpy model, which no libm gives
IR_DEVINL double det_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    int hx = (int)(bits >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i = (hx + 0x95f64) & 0x100000;
    const unsigned long long hi = (unsigned long long)(unsigned)(hx | (i ^ 0x3ff00000));
    const double xm = __longlong_as_double((long long)((hi << 32) | (bits & 0xffffffffull)));   // sqrt(2) / 2 <= xm < sqrt(2)
    k += i >> 20;
    const double f = xm - 1.0, s = f / (2.0 + f), dk = (double)k, z = s * s, w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1, hfsq = (0.5 * f) * f;
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
}

constexpr int LTPB = 1024, LWAVES = LTPB / 64;
// mean of log(c + 1e-5) of plane blockIdx.x (R, G, B) into means[blockIdx.x]: one workgroup of 1024 threads in the order of the block sums
// (thread t adds elements t, t + 1024, ...; a wave folds by xor 32 .. 1; the sixteen waves are added in turn)
__global__ __launch_bounds__(LTPB) void log_mean_kernel(const double* __restrict__ rgb, int N, double* __restrict__ means) {
    __shared__ double red[LWAVES];
    const long NN = (long)N * N;
    const double* p = rgb + blockIdx.x * NN;
    double a = 0.0;
    for (long i = threadIdx.x; i < NN; i += LTPB) a += det_log(p[i] + K_LOG);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int i = 1; i < LWAVES; ++i) s += red[i];
        means[blockIdx.x] = s / (double)NN;
    }
}

// planes 4-6
__global__ __launch_bounds__(256) void log_planes_kernel(const double* __restrict__ rgb, const double* __restrict__ means, int N, double* __restrict__ planes) {
    const long NN = (long)N * N, i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= NN) return;
    const double r = det_log(rgb[i] + K_LOG) - means[0], g = det_log(rgb[NN + i] + K_LOG) - means[1], b = det_log(rgb[2 * NN + i] + K_LOG) - means[2];
    planes[4 * NN + i] = (r + g + b) / sqrt(3.0);
    planes[5 * NN + i] = (r + g - 2.0 * b) / sqrt(6.0);
    planes[6 * NN + i] = (r - g) / sqrt(2.0);
}

// conv2(., 'same') with the two rank-one derivative kernels as two 11-tap passes (rows first), zero padding; a 32 x 32 tile per workgroup.
// mode 0: source blockIdx.z of the opponent planes -> Ix, Iy into planes 7 + 2 z, 8 + 2 z and sqrt(Ix^2 + Iy^2 + EPS) into plane 1 + z.
// mode 1: source plane 13 + z (a filter response) -> planes 37 + 2 z, 38 + 2 z and sqrt(dx^2 + dy^2) + EPS into plane 85 + z.
constexpr int DT = 32, DH = 5, DI = DT + 2 * DH;
__global__ __launch_bounds__(256) void deriv_kernel(const double* __restrict__ opp, double* __restrict__ planes, int N, int mode, Taps tp) {
    __shared__ double s_in[DI][DI + 1];
    __shared__ double s_x[DI][DT + 1], s_g[DI][DT + 1];
    const long NN = (long)N * N;
    const int z = blockIdx.z, x0 = blockIdx.x * DT, y0 = blockIdx.y * DT, tid = threadIdx.x;
    const double* src = mode == 0 ? opp + z * NN : planes + (13 + z) * NN;
    for (int i = tid; i < DI * DI; i += 256) {
        const int ly = i / DI, lx = i - ly * DI, gy = y0 - DH + ly, gx = x0 - DH + lx;
        s_in[ly][lx] = (gy >= 0 && gy < N && gx >= 0 && gx < N) ? src[(long)gy * N + gx] : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < DI * DT; i += 256) {
        const int ly = i / DT, lx = i - ly * DT;
        double ax = 0.0, ag = 0.0;
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            const double v = s_in[ly][lx + 10 - t];
            ax += tp.xg[t] * v;
            ag += tp.g[t] * v;
        }
        s_x[ly][lx] = ax;
        s_g[ly][lx] = ag;
    }
    __syncthreads();
    for (int i = tid; i < DT * DT; i += 256) {
        const int ly = i / DT, lx = i - ly * DT, gy = y0 + ly, gx = x0 + lx;
        if (gy >= N || gx >= N) continue;
        double dx = 0.0, dy = 0.0;
#pragma unroll
        for (int t = 0; t < 11; ++t) {
            dx += tp.g[t] * s_x[ly + 10 - t][lx];
            dy += tp.xg[t] * s_g[ly + 10 - t][lx];
        }
        const long at = (long)gy * N + gx;
        if (mode == 0) {
            planes[(7 + 2 * z) * NN + at] = dx;
            planes[(8 + 2 * z) * NN + at] = dy;
            planes[(1 + z) * NN + at] = sqrt(dx * dx + dy * dy + IL_EPS);
        } else {
            planes[(37 + 2 * z) * NN + at] = dx;
            planes[(38 + 2 * z) * NN + at] = dy;
            planes[(85 + z) * NN + at] = sqrt(dx * dx + dy * dy) + IL_EPS;
        }
    }
}

// ---- block statistics. Every sum is taken in ONE order, which the model restates: thread t of 256 adds elements t, t + 256, ... of the block
// (row-major) from 0.0, the 64 lanes of a wave fold by xor 32, 16, 8, 4, 2, 1, and the four waves are added in turn.
struct Six { double v[6]; };
IR_DEVINL void six_add(Six& a, double v) {
    const double sq = v * v;
    if (v < 0.0) {
        a.v[0] += 1.0;
        a.v[2] += sq;
    } else if (v > 0.0) {
        a.v[1] += 1.0;
        a.v[3] += sq;
    }
    a.v[4] += fabs(v);
    a.v[5] += sq;
}

// planes 7-84: blockIdx.x the block, blockIdx.y the plane - 7
__global__ __launch_bounds__(WTPB) void aggd_kernel(const double* __restrict__ planes, int N, int B, double* __restrict__ out) {
    __shared__ double s_red[WWAVES];
    const int per = N / B, tid = threadIdx.x;
    const double* blk = planes + (long)(7 + blockIdx.y) * N * N + (long)(blockIdx.x / per) * B * N + (blockIdx.x % per) * B;
    Six a{};
    for (int i = tid; i < B * B; i += WTPB) six_add(a, blk[(long)(i / B) * N + i % B]);
    double* o = out + (long)blockIdx.x * IR_ILNIQE_STATS + 30 + 6 * blockIdx.y;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double t = wg_sum(a.v[k], s_red);
        if (tid == 0) o[k] = t;
    }
}

// plane 0: the value and its four products with the neighbours taken circularly inside the block
__global__ __launch_bounds__(WTPB) void mscn_fields_kernel(const double* __restrict__ planes, int N, int B, double* __restrict__ out) {
    __shared__ double s_m[IR_WEIBULL_MAX];
    __shared__ double s_red[WWAVES];
    const int per = N / B, tid = threadIdx.x;
    const double* blk = planes + (long)(blockIdx.x / per) * B * N + (blockIdx.x % per) * B;
    for (int i = tid; i < B * B; i += WTPB) s_m[i] = blk[(long)(i / B) * N + i % B];
    __syncthreads();
    Six a[5] = {};
    for (int i = tid; i < B * B; i += WTPB) {
        const int py = i / B, px = i - py * B;
        const int pu = py == 0 ? B - 1 : py - 1, pl = px == 0 ? B - 1 : px - 1, pr = px == B - 1 ? 0 : px + 1;
        const double m = s_m[i];
        six_add(a[0], m);
        six_add(a[1], m * s_m[py * B + pl]);
        six_add(a[2], m * s_m[pu * B + px]);
        six_add(a[3], m * s_m[pu * B + pl]);
        six_add(a[4], m * s_m[pu * B + pr]);
    }
    double* o = out + (long)blockIdx.x * IR_ILNIQE_STATS;
#pragma unroll
    for (int f = 0; f < 5; ++f)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double t = wg_sum(a[f].v[k], s_red);
            if (tid == 0) o[6 * f + k] = t;
        }
}

// planes 4-6: mean and unbiased variance (two passes); blockIdx.y the plane - 4
__global__ __launch_bounds__(WTPB) void mean_var_kernel(const double* __restrict__ planes, int N, int B, double* __restrict__ out) {
    __shared__ double s_red[WWAVES];
    const int per = N / B, tid = threadIdx.x;
    const double* blk = planes + (long)(4 + blockIdx.y) * N * N + (long)(blockIdx.x / per) * B * N + (blockIdx.x % per) * B;
    double a = 0.0;
    for (int i = tid; i < B * B; i += WTPB) a += blk[(long)(i / B) * N + i % B];
    const double mean = wg_sum(a, s_red) / (double)(B * B);
    a = 0.0;
    for (int i = tid; i < B * B; i += WTPB) {
        const double d = blk[(long)(i / B) * N + i % B] - mean;
        a += d * d;
    }
    const double var = wg_sum(a, s_red) / (double)(B * B - 1);
    if (tid == 0) {
        out[(long)blockIdx.x * IR_ILNIQE_STATS + 498 + 2 * blockIdx.y] = mean;
        out[(long)blockIdx.x * IR_ILNIQE_STATS + 499 + 2 * blockIdx.y] = var;
    }
}

}  // namespace

void ir_ilniqe_twiddles_host(int N, double* cos_nn, double* sin_nn) {
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < N; ++j)
        for (int k = 0; k < N; ++k) {
            const int jk = (int)(((long)j * k) % N);   // reduced in integers first, so cos and sin see an argument below 2 pi
            cos_nn[(long)j * N + k] = std::cos(2.0 * pi * jk / N);
            sin_nn[(long)j * N + k] = std::sin(2.0 * pi * jk / N);
        }
}

int ir_launch_dft2_f64(const double* tw_cos, const double* tw_sin, const double* re, const double* im, int N, int inverse, double* out_re, double* out_im,
                       double* ws, hipStream_t s) {
    if ((N != 252 && N != 504) || !tw_cos || !tw_sin) return -1;
    const long NN = (long)N * N;
    const int tiles = (N + 31) / 32;
    const double wsign = inverse ? 1.0 : -1.0;   // forward: exp(-i ...)
    // T^T = (W X)^T into the workspace
    DftArgs p1{tw_cos, tw_sin, re, im, nullptr, ws, ws + NN, 0, 0, 0, N, 1, wsign, 1.0, 1.0};
    if (im) hipLaunchKernelGGL(dft_gemm_kernel<false>, dim3(tiles, tiles), dim3(64), 0, s, p1);
    else hipLaunchKernelGGL(dft_gemm_kernel<true>, dim3(tiles, tiles), dim3(64), 0, s, p1);
    // Y = T W
    DftArgs p2{ws, ws + NN, tw_cos, tw_sin, nullptr, out_re, out_im, 0, 0, 0, N, 0, 1.0, wsign, inverse ? 1.0 / ((double)N * N) : 1.0};
    hipLaunchKernelGGL(dft_gemm_kernel<false>, dim3(tiles, tiles), dim3(64), 0, s, p2);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int ir_launch_weibull_fit(const double* x, int rows, int count, double* k_lambda, hipStream_t s) {
    if (rows < 1 || count < 2 || count > IR_WEIBULL_MAX) return -1;
    hipLaunchKernelGGL(weibull_kernel, dim3(rows), dim3(WTPB), 0, s, x, count, k_lambda, 0, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------- ir_ilniqe_plan / ir_ilniqe_stats
int ir_ilniqe_taps(int n_in) {
    const double scale = (double)NS / n_in;
    return (int)std::ceil(scale < 1.0 ? 4.0 / scale : 4.0) + 2;
}

static double cubic(double x) {
    const double a = std::fabs(x);
    if (a <= 1.0) return (1.5 * a - 2.5) * a * a + 1.0;
    if (a <= 2.0) return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0;
    return 0.0;
}

// MATLAB's contributions() for n_in -> 524: idx [524][P] (0-based, symmetric padding), w [524][P] divided by their sum in tap order
static void resize_axis(int n_in, int* idx, double* w) {
    const double scale = (double)NS / n_in;
    const double width = scale < 1.0 ? 4.0 / scale : 4.0;
    const int P = ir_ilniqe_taps(n_in);
    for (int o = 0; o < NS; ++o) {
        const double u = (double)(o + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
        const double left = std::floor(u - width / 2.0);
        double total = 0.0;
        for (int t = 0; t < P; ++t) {
            const double d = u - (left + t);
            w[o * P + t] = scale < 1.0 ? scale * cubic(scale * d) : cubic(d);
            total = total + w[o * P + t];
            long m = ((long)left + t - 1) % (2L * n_in);
            if (m < 0) m += 2L * n_in;
            idx[o * P + t] = (int)(m < n_in ? m : 2L * n_in - 1 - m);
        }
        for (int t = 0; t < P; ++t) w[o * P + t] = w[o * P + t] / total;
    }
}

size_t ir_ilniqe_plan_layout(int h, int w, size_t* idx1, size_t* w0, size_t* w1) {
    const size_t P0 = ir_ilniqe_taps(h), P1 = ir_ilniqe_taps(w);
    *idx1 = NS * P0 * sizeof(int);
    *w0 = (*idx1 + NS * P1 * sizeof(int) + 7) & ~(size_t)7;
    *w1 = *w0 + NS * P0 * sizeof(double);
    return *w1 + NS * P1 * sizeof(double);
}

void ir_ilniqe_plan_host(int h, int w, void* tables) {
    size_t i1, w0, w1;
    ir_ilniqe_plan_layout(h, w, &i1, &w0, &w1);
    char* b = static_cast<char*>(tables);
    resize_axis(h, reinterpret_cast<int*>(b), reinterpret_cast<double*>(b + w0));
    resize_axis(w, reinterpret_cast<int*>(b + i1), reinterpret_cast<double*>(b + w1));
}

size_t ir_ilniqe_workspace(int w) {
    const size_t NN = (size_t)N1 * N1;
    return ((size_t)N1 * 3 * w + 6 * NN + 6 * NN / 4 + 2 * NN + 109 * NN + 32) * sizeof(double);
}

int ir_launch_ilniqe_stats(const IrIlniqeTables& tb, const uint8_t* img, int rows, long pitch, int n, int h, int w, const void* plan, double* out,
                           double* ws, hipStream_t s) {
    if (n < 1 || h < 2 || w < 2 || !tb.ok) return -1;
    const long NN1 = (long)N1 * N1;
    size_t i1, o0, o1;
    ir_ilniqe_plan_layout(h, w, &i1, &o0, &o1);
    const char* pb = static_cast<const char*>(plan);
    const Plan pl{reinterpret_cast<const int*>(pb), reinterpret_cast<const int*>(pb + i1), reinterpret_cast<const double*>(pb + o0),
                  reinterpret_cast<const double*>(pb + o1), ir_ilniqe_taps(h), ir_ilniqe_taps(w)};
    double* tmp = ws;
    double* rgbo1 = tmp + (size_t)N1 * 3 * w;
    double* rgbo2 = rgbo1 + 6 * NN1;
    double* F = rgbo2 + 6 * NN1 / 4;
    double* planes = F + 2 * NN1;
    double* means = planes + 109 * NN1;
    Win5 w5;
    Win6 w6;
    for (int i = 0; i < 25; ++i) w5.k[i] = tb.win5[i];
    for (int i = 0; i < 36; ++i) w6.k[i] = tb.win6[i];
    const int w3 = 3 * w;
    for (int image = 0; image < n; ++image) {
        const uint8_t* src = img + (long)image * rows * pitch;
        hipLaunchKernelGGL(resize_cols_kernel, dim3((w3 + 255) / 256, N1), dim3(256), 0, s, src, pitch, w3, pl, tmp);
        hipLaunchKernelGGL(resize_rows_kernel, dim3((N1 + 255) / 256, N1), dim3(256), 0, s, tmp, w3, pl, rgbo1);
        hipLaunchKernelGGL(down6_kernel, dim3(1, N1 / 2, 6), dim3(256), 0, s, rgbo1, rgbo2, N1, w6);
        for (int sc = 0; sc < 2; ++sc) {
            const int N = N1 >> sc, B = IR_ILNIQE_BLOCK >> sc, tiles = (N + 31) / 32, dt = (N + DT - 1) / DT;
            const long NN = (long)N * N;
            const double* rgbo = sc ? rgbo2 : rgbo1;
            const double *tc = tb.tw[1 - sc], *ts = tc + NN;
            Taps tp;
            for (int i = 0; i < 11; ++i) {
                tp.xg[i] = tb.taps[sc][i];
                tp.g[i] = tb.taps[sc][11 + i];
            }
            hipLaunchKernelGGL(mscn_kernel, dim3((N + 255) / 256, N), dim3(256), 0, s, rgbo + 5 * NN, planes, N, w5);
            hipLaunchKernelGGL(log_mean_kernel, dim3(3), dim3(LTPB), 0, s, rgbo, N, means);
            hipLaunchKernelGGL(log_planes_kernel, dim3((unsigned)((NN + 255) / 256)), dim3(256), 0, s, rgbo, means, N, planes);
            hipLaunchKernelGGL(deriv_kernel, dim3(dt, dt, 3), dim3(256), 0, s, rgbo + 3 * NN, planes, N, 0, tp);
            // F = fft2(O3), its column transform in planes 37-38; then the twelve responses: the column transforms (W^* (F_f . F))^T in planes
            // 37-60, the responses into planes 13-36 (Re, Im of filter f at 13 + 2 f, 14 + 2 f)
            if (ir_launch_dft2_f64(tc, ts, rgbo + 5 * NN, nullptr, N, 0, F, F + NN, planes + 37 * NN, s)) return -1;
            DftArgs p1{tc, ts, F, F + NN, tb.bank[1 - sc], planes + 37 * NN, planes + 38 * NN, 0, NN, 2 * NN, N, 1, 1.0, 1.0, 1.0};
            hipLaunchKernelGGL(dft_gemm_kernel<false>, dim3(tiles, tiles, 12), dim3(64), 0, s, p1);
            DftArgs p2{planes + 37 * NN, planes + 38 * NN, tc, ts, nullptr, planes + 13 * NN, planes + 14 * NN, 2 * NN, 0, 2 * NN, N, 0, 1.0, 1.0,
                       1.0 / ((double)N * N)};
            hipLaunchKernelGGL(dft_gemm_kernel<false>, dim3(tiles, tiles, 12), dim3(64), 0, s, p2);
            hipLaunchKernelGGL(deriv_kernel, dim3(dt, dt, 24), dim3(256), 0, s, rgbo, planes, N, 1, tp);
            double* o = out + ((long)image * 2 + sc) * 36 * IR_ILNIQE_STATS;
            hipLaunchKernelGGL(mscn_fields_kernel, dim3(36), dim3(WTPB), 0, s, planes, N, B, o);
            hipLaunchKernelGGL(aggd_kernel, dim3(36, 78), dim3(WTPB), 0, s, planes, N, B, o);
            hipLaunchKernelGGL(mean_var_kernel, dim3(36, 3), dim3(WTPB), 0, s, planes, N, B, o);
            hipLaunchKernelGGL(weibull_kernel, dim3(36, 27), dim3(WTPB), 0, s, planes, B * B, o, B, N);
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
