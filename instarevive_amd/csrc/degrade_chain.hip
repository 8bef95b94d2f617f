// The second-order degradation chain on device images (ir_degrade_chain): the definition of tools/degrade_folder.py:degrade_chain_model - the
// Real-ESRGAN recipe of the reference's dataset/realesrgan.py and dataset/batch_transform.py:RealESRGANBatchTransform, as a list of ops on a
// float32 [h][w][3] image - in the model's order of operations, so the bytes and every intermediate float equal the model's.
// One image is a chain of launches on the stream through two float images of the workspace (the images of a batch follow each other):
//   load     x = float32(v / 255.0)
//   filter   utils/image/common.py:filter2D: the halo tile of a 32 x 32 patch (reflect border) as three float planes in LDS (52 x 52 x 3 x 4 B =
//            32 KB for K = 21, the largest K taken); every thread owns four pixels and adds k * x to its twelve fp64 accumulators in row-major
//            tap order, multiply and add apart; rounded once to float32.
//   resize   F.interpolate without antialiasing, one kernel per mode, one thread per output pixel. The source coordinate is
//            float32(s * (float32(d) + 0.5) - 0.5) with the product and the difference in double (torch's CPU kernels fuse them), s =
//            float32(1 / scale_factor) or float32(in) / float32(out); bilinear clamps a negative coordinate to 0, bicubic (A = -0.75, weights in
//            float32) clamps its indices; area is adaptive_avg_pool2d's window. Taps summed in fp64 in row-major order, rounded once.
//   gauss    x + n * sigma / 255 in float32, clip to [0, 1]; gray: one field value for the three channels. In place.
//   poisson  levels: the level clip(rint(x * 255)) of every value (gray: of (0.2989 R + 0.587 G) + 0.114 B) marks a 256-entry presence array
//            with a plain store; draw: every workgroup counts the marks (vals = the power of two at or above), then lambda = level / 255 * vals,
//            p = exp(-lambda) from the caller's table, the inversion loop in fp64 against the caller's uniform field, and
//            x + (k / vals - r) * scale, clip. No floating-point atomics, no atomics at all. In place.
//   diffjpeg utils/image/diffjpeg.py: ycc (clamp, * 255, the float32 colour matrix as an fp64 3-term sum, zero padding to multiples of 16,
//            the 2 x 2 chroma mean) into float planes; dct: a workgroup takes 16 blocks of 8 x 8, four at a time, one thread per coefficient,
//            the caller's basis [64][64] in LDS (rows padded to 65 doubles: the forward pass walks it by columns, the inverse by rows) - the
//            64-term forward sum, * scale, / (table * factor), rint, * (table * factor), * alpha, the 64-term inverse sum, 0.25 * sum + 128, in
//            place; rgb: replicated chroma, - 128, the inverse matrix, the clamp, / 255, the crop.
//   finish   uint8(clip(rint(x * 255), 0, 255)), half to even.
// The order of the floating-point operations is the definition, so build.py compiles this file with -ffp-contract=off like degrade.hip.
#include <math.h>

#include <utility>

#include "../../include/instarevive_hip.h"
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int PATCH = 32;   // the filter's output patch of a workgroup: 32 columns x (8 threads x 4 rows)
constexpr int MAX_K = IR_CHAIN_MAX_KSIZE;
constexpr int POISSON_MAX_K = 1024;
constexpr int DCT_ROUNDS = 4;   // a dct workgroup takes DCT_ROUNDS x 4 blocks
constexpr int BASIS_ROW = 65;

IR_DEVINL int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
IR_DEVINL float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }
IR_DEVINL int reflect101(int i, int n) { return clampi(i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i), 0, n - 1); }
IR_DEVINL int level_of(float v) { return clampi((int)rintf(v * 255.0f), 0, 255); }
IR_DEVINL float over255(float v) { return (float)((double)v / 255.0); }   // the float32 quotient: a double quotient rounds to it

// ---------------------------------------------------------------- load, finish
__global__ __launch_bounds__(TPB) void chain_load_kernel(const uint8_t* __restrict__ img, long pitch, int h, int w, float* __restrict__ out) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const uint8_t* p = img + (long)y * pitch + 3L * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = over255((float)p[c]);
}

__global__ __launch_bounds__(TPB) void chain_finish_kernel(const float* __restrict__ src, int h, int w, uint8_t* __restrict__ out, long pitch) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    uint8_t* p = out + (long)y * pitch + 3L * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = (uint8_t)level_of(src[i * 3 + c]);
}

// ---------------------------------------------------------------- filter
__global__ __launch_bounds__(TPB) void chain_filter_kernel(const float* __restrict__ src, int h, int w, const double* __restrict__ k, int K,
                                                           float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float chain_tile[];   // [3][T][T]
    const int R = K >> 1, T = PATCH + K - 1, tid = threadIdx.x;
    const int x0 = blockIdx.x * PATCH, y0 = blockIdx.y * PATCH;
    for (int i = tid; i < T * T; i += TPB) {
        const int ly = i / T, lx = i - ly * T;
        const float* p = src + ((long)reflect101(y0 - R + ly, h) * w + reflect101(x0 - R + lx, w)) * 3;
        chain_tile[i] = p[0];
        chain_tile[T * T + i] = p[1];
        chain_tile[2 * T * T + i] = p[2];
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    double acc[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0;
    for (int a = 0; a < K; ++a)
        for (int b = 0; b < K; ++b) {
            const double kv = k[a * K + b];   // the same address in every lane
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int at = (ty + 8 * j + a) * T + tx + b;
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[j][c] += kv * (double)chain_tile[c * T * T + at];
            }
        }
    const int x = x0 + tx;
    if (x >= w) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = y0 + ty + 8 * j;
        if (y < h) {
            float* o = out + ((long)y * w + x) * 3;
            o[0] = (float)acc[j][0];
            o[1] = (float)acc[j][1];
            o[2] = (float)acc[j][2];
        }
    }
}

// ---------------------------------------------------------------- resize
IR_DEVINL float src_coord(int d, float s) { return (float)((double)s * (double)((float)d + 0.5f) - 0.5); }

struct Lin {
    int i[2];
    float w[2];
};

IR_DEVINL Lin lin_taps(int d, int src, float s) {
    float real = src_coord(d, s);
    if (real < 0.0f) real = 0.0f;
    int i0 = (int)real;
    if (i0 > src - 1) i0 = src - 1;
    const float lam = clampf(real - (float)i0, 0.0f, 1.0f);
    return Lin{{i0, i0 + (i0 < src - 1 ? 1 : 0)}, {1.0f - lam, lam}};
}

struct Cub {
    int i[4];
    float w[4];
};

IR_DEVINL float cub_near(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.0f; }                 // ((A + 2) x - (A + 3)) x x + 1, A = -0.75
IR_DEVINL float cub_far(float x) { return ((-0.75f * x - (-3.75f)) * x + (-6.0f)) * x - (-3.0f); }   // ((A x - 5 A) x + 8 A) x - 4 A

IR_DEVINL Cub cub_taps(int d, int src, float s) {
    const float real = src_coord(d, s), fl = floorf(real);
    const float t = clampf(real - fl, 0.0f, 1.0f), u = 1.0f - t;
    const int i = (int)fl;
    return Cub{{clampi(i - 1, 0, src - 1), clampi(i, 0, src - 1), clampi(i + 1, 0, src - 1), clampi(i + 2, 0, src - 1)},
               {cub_far(t + 1.0f), cub_near(t), cub_near(u), cub_far(u + 1.0f)}};
}

__global__ __launch_bounds__(TPB) void chain_bilinear_kernel(const float* __restrict__ src, int sh, int sw, int oh, int ow, float sy, float sx,
                                                             float* __restrict__ dst) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)oh * ow) return;
    const int dy = (int)(i / ow), dx = (int)(i - (long)dy * ow);
    const Lin ty = lin_taps(dy, sh, sy), tx = lin_taps(dx, sw, sx);
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double wgt = (double)ty.w[a] * (double)tx.w[b];
            const float* p = src + ((long)ty.i[a] * sw + tx.i[b]) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wgt * (double)p[c];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (float)acc[c];
}

__global__ __launch_bounds__(TPB) void chain_bicubic_kernel(const float* __restrict__ src, int sh, int sw, int oh, int ow, float sy, float sx,
                                                            float* __restrict__ dst) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)oh * ow) return;
    const int dy = (int)(i / ow), dx = (int)(i - (long)dy * ow);
    const Cub ty = cub_taps(dy, sh, sy), tx = cub_taps(dx, sw, sx);
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const double wgt = (double)ty.w[a] * (double)tx.w[b];
            const float* p = src + ((long)ty.i[a] * sw + tx.i[b]) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wgt * (double)p[c];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (float)acc[c];
}

__global__ __launch_bounds__(TPB) void chain_area_kernel(const float* __restrict__ src, int sh, int sw, int oh, int ow, float* __restrict__ dst) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)oh * ow) return;
    const int dy = (int)(i / ow), dx = (int)(i - (long)dy * ow);
    const int y0 = (int)(((long)dy * sh) / oh), y1 = (int)((((long)dy + 1) * sh + oh - 1) / oh);
    const int x0 = (int)(((long)dx * sw) / ow), x1 = (int)((((long)dx + 1) * sw + ow - 1) / ow);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const float* p = src + ((long)y * sw + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (double)p[c];
        }
    const double count = (double)((long)(y1 - y0) * (x1 - x0));
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (float)(acc[c] / count);
}

// ---------------------------------------------------------------- noise
__global__ __launch_bounds__(TPB) void chain_gauss_kernel(float* __restrict__ x, long npx, const float* __restrict__ field, float sigma, int gray) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npx) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float n = gray ? field[i] : field[i * 3 + c];
        x[i * 3 + c] = clampf(x[i * 3 + c] + n * sigma / 255.0f, 0.0f, 1.0f);
    }
}

IR_DEVINL float gray_of(const float* p) { return (0.2989f * p[0] + 0.587f * p[1]) + 0.114f * p[2]; }

__global__ __launch_bounds__(TPB) void chain_levels_kernel(const float* __restrict__ x, long npx, int gray, int* __restrict__ present) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npx) return;
    if (gray) {
        present[level_of(gray_of(x + i * 3))] = 1;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) present[level_of(x[i * 3 + c])] = 1;
    }
}

// p(0) = p0, p(k + 1) = p(k) * lam / (k + 1): the smallest k whose cumulative sum exceeds u
IR_DEVINL int poisson_invert(double lam, double p, double u) {
    double cum = p;
    int k = 0;
    while (cum <= u && k < POISSON_MAX_K) {
        ++k;
        p = p * lam / (double)k;
        cum = cum + p;
    }
    return k;
}

__global__ __launch_bounds__(TPB) void chain_poisson_kernel(float* __restrict__ x, long npx, int gray, const double* __restrict__ u, float scale,
                                                            const int* __restrict__ present, const double* __restrict__ exp_table) {
    static_assert(TPB == 256, "one thread per level");
    const int count = __syncthreads_count(present[threadIdx.x] != 0);
    int vals = 1, lg = 0;
    while (vals < count) vals *= 2, ++lg;
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= npx) return;
    const float fv = (float)vals;
    if (gray) {
        const int lv = level_of(gray_of(x + i * 3));
        const float r = over255((float)lv);
        const int k = poisson_invert((double)(r * fv), exp_table[lg * 256 + lv], u[i]);
        const float noise = ((float)k / fv - r) * scale;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[i * 3 + c] = clampf(x[i * 3 + c] + noise, 0.0f, 1.0f);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = x[i * 3 + c];
            const int lv = level_of(v);
            const float r = over255((float)lv);
            const int k = poisson_invert((double)(r * fv), exp_table[lg * 256 + lv], u[i * 3 + c]);
            x[i * 3 + c] = clampf(v + ((float)k / fv - r) * scale, 0.0f, 1.0f);
        }
    }
}

// ---------------------------------------------------------------- DiffJPEG
struct Mat3 {
    float m[3][3];   // [out][in]
    float shift[3];
};
constexpr Mat3 RGB_TO_YCC = {{{0.299f, 0.587f, 0.114f}, {-0.168736f, -0.331264f, 0.5f}, {0.5f, -0.418688f, -0.081312f}}, {0.0f, 128.0f, 128.0f}};
constexpr Mat3 YCC_TO_RGB = {{{1.0f, 0.0f, 1.402f}, {1.0f, -0.344136f, -0.714136f}, {1.0f, 1.772f, 0.0f}}, {0.0f, 0.0f, 0.0f}};

IR_DEVINL float dot3(const float m[3], double a, double b, double c) { return (float)(((double)m[0] * a + (double)m[1] * b) + (double)m[2] * c); }

// one thread per chroma sample of the padded planes: its 2 x 2 luma samples and its Cb and Cr
__global__ __launch_bounds__(TPB) void chain_ycc_kernel(const float* __restrict__ x, int h, int w, int PH, int PW, float* __restrict__ Y,
                                                        float* __restrict__ Cb, float* __restrict__ Cr, Mat3 mat) {
    const int CW = PW >> 1, CH = PH >> 1;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= CW * CH) return;
    const int cy = i / CW, cx = i - cy * CW;
    double cb = 0.0, cr = 0.0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int py = 2 * cy + dy, px = 2 * cx + dx;
            double v[3] = {0.0, 0.0, 0.0};   // the padding is zero BEFORE the colour matrix
            if (py < h && px < w) {
                const float* p = x + ((long)py * w + px) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (double)(clampf(p[c], 0.0f, 1.0f) * 255.0f);
            }
            float ycc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                ycc[c] = (float)((((double)mat.m[c][0] * v[0] + (double)mat.m[c][1] * v[1]) + (double)mat.m[c][2] * v[2]) + (double)mat.shift[c]);
            Y[(long)py * PW + px] = ycc[0];
            cb = (dy == 0 && dx == 0) ? (double)ycc[1] : cb + (double)ycc[1];
            cr = (dy == 0 && dx == 0) ? (double)ycc[2] : cr + (double)ycc[2];
        }
    Cb[i] = (float)(cb / 4.0);
    Cr[i] = (float)(cr / 4.0);
}

struct JpegTables {
    uint8_t t[2][64];   // libjpeg's luminance and chrominance tables, natural order; the module's are their transposes
};

// planes [gridDim.y][H][W] floats, H and W multiples of 8, in place. tables: the caller's [64][64] basis, [64] scale, [64] alpha (doubles).
__global__ __launch_bounds__(TPB) void chain_dct_kernel(float* __restrict__ planes, int H, int W, const double* __restrict__ tables, float factor,
                                                        JpegTables qt, int table) {
    __shared__ double s_basis[64 * BASIS_ROW];
    __shared__ double s_v[4][64];
    for (int i = threadIdx.x; i < 64 * 64; i += TPB) s_basis[(i >> 6) * BASIS_ROW + (i & 63)] = tables[i];
    const int g = threadIdx.x >> 6, e = threadIdx.x & 63;
    const double scale = tables[4096 + e];
    const float alpha = (float)tables[4096 + 64 + e];
    const float tf = (float)qt.t[table][(e & 7) * 8 + (e >> 3)] * factor;   // the transposed table
    const int bw = W >> 3, nblk = bw * (H >> 3);
    float* plane = planes + (long)blockIdx.y * H * W;
    for (int r = 0; r < DCT_ROUNDS; ++r) {
        const int blk = (blockIdx.x * DCT_ROUNDS + r) * 4 + g;
        const bool live = blk < nblk;
        const int by = live ? blk / bw : 0, bx = live ? blk - by * bw : 0;
        float* px = plane + (long)(by * 8 + (e >> 3)) * W + bx * 8 + (e & 7);
        __syncthreads();   // the basis (first round); the previous round's readers of s_v
        s_v[g][e] = live ? (double)*px - 128.0 : 0.0;
        __syncthreads();
        double acc = 0.0;
        for (int s = 0; s < 64; ++s) acc += s_v[g][s] * s_basis[s * BASIS_ROW + e];   // thread e: frequency e
        const float coef = (float)(scale * acc);
        const float q = rintf((float)((double)coef / (double)tf));
        const float back = (q * tf) * alpha;
        __syncthreads();
        s_v[g][e] = (double)back;
        __syncthreads();
        acc = 0.0;
        for (int f = 0; f < 64; ++f) acc += s_v[g][f] * s_basis[e * BASIS_ROW + f];   // thread e: sample e
        if (live) *px = (float)(0.25 * acc + 128.0);
    }
}

__global__ __launch_bounds__(TPB) void chain_rgb_kernel(const float* __restrict__ Y, const float* __restrict__ Cb, const float* __restrict__ Cr, int PW,
                                                        int h, int w, float* __restrict__ out, Mat3 mat) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const long ci = (long)(y >> 1) * (PW >> 1) + (x >> 1);
    const double yy = (double)Y[(long)y * PW + x], cb = (double)(Cb[ci] - 128.0f), cr = (double)(Cr[ci] - 128.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = over255(clampf(dot3(mat.m[c], yy, cb, cr), 0.0f, 255.0f));
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t a, b, y, c, present, total;
};

Layout layout(int mh, int mw) {
    const size_t PH = (size_t)(mh + 15) & ~(size_t)15, PW = (size_t)(mw + 15) & ~(size_t)15;
    Layout l;
    size_t at = 0;
    l.a = at, at += up256((size_t)mh * mw * 3 * sizeof(float));
    l.b = at, at += up256((size_t)mh * mw * 3 * sizeof(float));
    l.y = at, at += up256(PH * PW * sizeof(float));
    l.c = at, at += up256(PH * PW / 2 * sizeof(float));   // Cb and Cr lie behind each other: one dct launch takes both
    l.present = at, at += up256(256 * sizeof(int));
    l.total = at;
    return l;
}

unsigned blocks(long n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

int ir_degrade_chain_check(const ir_chain* ch, int h, int w, int* max_ih, int* max_iw, const char** why) {
    int ih = h, iw = w, mh = h, mw = w;
    *why = "";
    if (ch->n_ops < 0 || ch->n_ops > IR_CHAIN_MAX_OPS) return *why = "more than 16 ops", -1;
    if (ch->tap < -1 || ch->tap >= ch->n_ops) return *why = "tap is not an op's index or -1", -1;
    for (int i = 0; i < ch->n_ops; ++i) {
        const ir_chain_op& op = ch->ops[i];
        switch (op.kind) {
        case IR_CHAIN_FILTER:
            if (op.a < 1 || op.a > MAX_K || !(op.a & 1)) return *why = "a filter size that is even or above 21", -1;
            if (ih < op.a / 2 + 1 || iw < op.a / 2 + 1) return *why = "an image too small for its filter (the reflection would leave it)", -1;
            if (!op.data || (reinterpret_cast<uintptr_t>(op.data) & 7)) return *why = "a filter without an aligned kernel", -1;
            break;
        case IR_CHAIN_RESIZE:
            if (op.a != IR_CHAIN_AREA && op.a != IR_CHAIN_BILINEAR && op.a != IR_CHAIN_BICUBIC) return *why = "an unknown resize mode", -1;
            if (op.b < 1 || op.c < 1 || op.b > IR_CHAIN_MAX_SIDE || op.c > IR_CHAIN_MAX_SIDE) return *why = "a resize to a size outside 1 .. 8192", -1;
            if (!(op.s >= 0.0)) return *why = "a negative scale factor", -1;
            if (op.s > 0.0 && ((double)op.b != floor((double)ih * op.s) || (double)op.c != floor((double)iw * op.s)))
                return *why = "a resize by a scale factor whose output size is not floor(in * scale)", -1;
            ih = op.b, iw = op.c;
            mh = ih > mh ? ih : mh, mw = iw > mw ? iw : mw;
            break;
        case IR_CHAIN_GAUSS:
        case IR_CHAIN_POISSON:
            if (!op.data || (reinterpret_cast<uintptr_t>(op.data) & (op.kind == IR_CHAIN_GAUSS ? 3 : 7))) return *why = "a noise op without an aligned field", -1;
            if (!(op.s >= 0.0)) return *why = "a negative noise level", -1;
            if (op.kind == IR_CHAIN_POISSON && (!ch->exp_table || (reinterpret_cast<uintptr_t>(ch->exp_table) & 7)))
                return *why = "Poisson noise without an aligned exp table", -1;
            break;
        case IR_CHAIN_DIFFJPEG:
            if (!(op.s > 0.0)) return *why = "a JPEG factor that is not positive", -1;
            if (!ch->dct_basis || (reinterpret_cast<uintptr_t>(ch->dct_basis) & 7)) return *why = "DiffJPEG without an aligned basis", -1;
            break;
        default:
            return *why = "an unknown op kind", -1;
        }
    }
    if (ih != h || iw != w) return *why = "a chain that does not end at the image's size", -1;
    *max_ih = mh, *max_iw = mw;
    return 0;
}

size_t ir_degrade_chain_workspace(int h, int w, int max_ih, int max_iw) {
    if (h < 1 || w < 1 || h > IR_CHAIN_MAX_SIDE || w > IR_CHAIN_MAX_SIDE || max_ih > IR_CHAIN_MAX_SIDE || max_iw > IR_CHAIN_MAX_SIDE) return 0;
    return layout(max_ih > h ? max_ih : h, max_iw > w ? max_iw : w).total;
}

int ir_launch_degrade_chain(const uint8_t* img, long pitch, int h, int w, const ir_chain* ch, int max_ih, int max_iw, uint8_t* out, long out_pitch,
                            float* tap, void* ws, hipStream_t s) {
    const Layout l = layout(max_ih > h ? max_ih : h, max_iw > w ? max_iw : w);
    uint8_t* base = static_cast<uint8_t*>(ws);
    float* cur = reinterpret_cast<float*>(base + l.a);
    float* nxt = reinterpret_cast<float*>(base + l.b);
    float* Y = reinterpret_cast<float*>(base + l.y);
    float* C = reinterpret_cast<float*>(base + l.c);
    int* present = reinterpret_cast<int*>(base + l.present);
    static const JpegTables qt = {{{16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
                                   {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}}};
    int ih = h, iw = w;
    hipLaunchKernelGGL(chain_load_kernel, dim3(blocks((long)h * w)), dim3(TPB), 0, s, img, pitch, h, w, cur);
    for (int i = 0; i < ch->n_ops; ++i) {
        const ir_chain_op& op = ch->ops[i];
        const long npx = (long)ih * iw;
        switch (op.kind) {
        case IR_CHAIN_FILTER: {
            const int T = PATCH + op.a - 1;
            static_assert((size_t)(PATCH + MAX_K - 1) * (PATCH + MAX_K - 1) * 12 <= 64 * 1024, "the filter's halo tile must fit in LDS");
            hipLaunchKernelGGL(chain_filter_kernel, dim3((iw + PATCH - 1) / PATCH, (ih + PATCH - 1) / PATCH), dim3(TPB), (size_t)T * T * 3 * sizeof(float), s,
                               cur, ih, iw, static_cast<const double*>(op.data), op.a, nxt);
            std::swap(cur, nxt);
            break;
        }
        case IR_CHAIN_RESIZE: {
            const int oh = op.b, ow = op.c;
            const float sy = op.s > 0.0 ? (float)(1.0 / op.s) : (float)ih / (float)oh, sx = op.s > 0.0 ? (float)(1.0 / op.s) : (float)iw / (float)ow;
            const dim3 grid(blocks((long)oh * ow));
            if (op.a == IR_CHAIN_AREA)
                hipLaunchKernelGGL(chain_area_kernel, grid, dim3(TPB), 0, s, cur, ih, iw, oh, ow, nxt);
            else if (op.a == IR_CHAIN_BILINEAR)
                hipLaunchKernelGGL(chain_bilinear_kernel, grid, dim3(TPB), 0, s, cur, ih, iw, oh, ow, sy, sx, nxt);
            else
                hipLaunchKernelGGL(chain_bicubic_kernel, grid, dim3(TPB), 0, s, cur, ih, iw, oh, ow, sy, sx, nxt);
            std::swap(cur, nxt);
            ih = oh, iw = ow;
            break;
        }
        case IR_CHAIN_GAUSS:
            hipLaunchKernelGGL(chain_gauss_kernel, dim3(blocks(npx)), dim3(TPB), 0, s, cur, npx, static_cast<const float*>(op.data), (float)op.s, op.a != 0);
            break;
        case IR_CHAIN_POISSON:
            if (hipMemsetAsync(present, 0, 256 * sizeof(int), s) != hipSuccess) return -1;
            hipLaunchKernelGGL(chain_levels_kernel, dim3(blocks(npx)), dim3(TPB), 0, s, cur, npx, op.a != 0, present);
            hipLaunchKernelGGL(chain_poisson_kernel, dim3(blocks(npx)), dim3(TPB), 0, s, cur, npx, op.a != 0, static_cast<const double*>(op.data), (float)op.s,
                               present, ch->exp_table);
            break;
        case IR_CHAIN_DIFFJPEG: {
            const int PH = (ih + 15) & ~15, PW = (iw + 15) & ~15;
            float *Cb = C, *Cr = C + (size_t)PH * PW / 4;   // the planes of THIS size, Cr right behind Cb
            constexpr int PER = DCT_ROUNDS * 4;
            hipLaunchKernelGGL(chain_ycc_kernel, dim3(blocks((long)PH * PW / 4)), dim3(TPB), 0, s, cur, ih, iw, PH, PW, Y, Cb, Cr, RGB_TO_YCC);
            hipLaunchKernelGGL(chain_dct_kernel, dim3((PH * PW / 64 + PER - 1) / PER, 1), dim3(TPB), 0, s, Y, PH, PW, ch->dct_basis, (float)op.s, qt, 0);
            hipLaunchKernelGGL(chain_dct_kernel, dim3((PH * PW / 256 + PER - 1) / PER, 2), dim3(TPB), 0, s, Cb, PH / 2, PW / 2, ch->dct_basis, (float)op.s, qt, 1);
            hipLaunchKernelGGL(chain_rgb_kernel, dim3(blocks(npx)), dim3(TPB), 0, s, Y, Cb, Cr, PW, ih, iw, cur, YCC_TO_RGB);
            break;
        }
        default:
            return -1;
        }
        if (tap && ch->tap == i && hipMemcpyAsync(tap, cur, (size_t)ih * iw * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
    }
    hipLaunchKernelGGL(chain_finish_kernel, dim3(blocks((long)h * w)), dim3(TPB), 0, s, cur, h, w, out, out_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
