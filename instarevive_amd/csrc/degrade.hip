// Low-quality inputs from ground truth on uint8 HWC RGB device images (ir_degrade): the definition of tools/degrade_folder.py - the first-order
// chain of the reference's dataset/codeformer.py:140-163 and tools/lq.py - in the model's order of operations, so the bytes equal the model's.
// One image is a chain of launches on the stream (the images of a batch follow each other through one workspace):
//   blur     x = float32(v / 255.0) of a 32 x 32 patch with the halo of the K x K kernel (BORDER_REFLECT_101) as three float planes in LDS
//            (72 x 72 x 3 x 4 B = 62 KB for K = 41, the largest K taken); every thread owns four pixels, reads the tap k[a][b] through a uniform (scalar) load and
//            adds k * x to its twelve fp64 accumulators in row-major tap order, multiply and add apart; rounded once to float32.
//   down     cv2.resize INTER_LINEAR on floats to lh x lw: fx = float32((dx + 0.5) * (w / lw) - 0.5) with the product in double, the two-tap
//            row pass on two source rows, then the two-tap column pass, all float32; then x += n * sigma / 255 and the clip to [0, 1].
//   ycc      (q > 0) bytes rint(x * 255), libjpeg's RGB -> YCbCr (jccolor.c) into 16-padded planes, the h2v2 chroma downsample with its
//            alternating bias and libjpeg's edge rules: Y and the full-resolution chroma columns replicate out to the padding, the
//            full-resolution chroma rows only to an even count, then the last DOWNSAMPLED row replicates.
//   dct      eight lanes per 8 x 8 block, in place: jfdctint.c along the rows and down the columns, quantise and dequantise, jidctint.c down
//            the columns and along the rows, + 128, clamp. Products of the 13-bit constants are summed in 64-bit integers (libjpeg's JLONG):
//            the second inverse pass can pass 31 bits on extreme coefficients.
//   rgb      h2v2 fancy upsampling on the true chroma size ceil(lh / 2) x ceil(lw / 2), YCbCr -> RGB (jdcolor.c), x = float32(byte) / 255.
//   up       the bilinear resize back to h x w and uint8(trunc(clip(x, 0, 1) * 255)); with norm = max the floats are kept, every workgroup
//            writes the maximum of its patch, one workgroup folds those in a fixed order (no floating-point atomics), and a last launch
//            writes uint8(trunc(max(x, 0) / m * 255)).
// The order of the floating-point operations is part of the definition (a byte is a truncation or a rounding of their result), so build.py
// compiles this file with -ffp-contract=off, for the reason niqe.hip gives: the pragma alone does not hold under -ffp-contract=fast.
#include "common.h"
#include "jpeg_back.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

using namespace ir_jpeg_back;

constexpr int TPB = 256;
constexpr int NORM_MAX = 1;   // IR_DEGRADE_NORM_MAX of include/instarevive_hip.h
constexpr int PATCH = 32;   // the blur's and the last resize's output patch of a workgroup: 32 columns x (8 threads x 4 rows)

IR_DEVINL float unit(int v) { return (float)((double)v / 255.0); }   // float32(v / 255.0); equals float32(v) / float32(255) for all 256 bytes
IR_DEVINL int reflect101(int i, int n) { return clampi(i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i), 0, n - 1); }

// ---------------------------------------------------------------- blur
__global__ __launch_bounds__(TPB) void degrade_blur_kernel(const uint8_t* __restrict__ img, long pitch, int h, int w, const double* __restrict__ k,
                                                           int K, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float deg_smem[];   // float32(v / 255.0) of the 256 bytes, then the tile [3][T][T]
    float* deg_tile = deg_smem + 256;
    const int R = K >> 1, T = PATCH + K - 1, tid = threadIdx.x;
    const int x0 = blockIdx.x * PATCH, y0 = blockIdx.y * PATCH;
    static_assert(TPB == 256, "one thread per byte value");
    deg_smem[tid] = unit(tid);
    __syncthreads();
    for (int i = tid; i < T * T; i += TPB) {
        const int ly = i / T, lx = i - ly * T;
        const uint8_t* p = img + (long)reflect101(y0 - R + ly, h) * pitch + 3L * reflect101(x0 - R + lx, w);
        deg_tile[i] = deg_smem[p[0]];
        deg_tile[T * T + i] = deg_smem[p[1]];
        deg_tile[2 * T * T + i] = deg_smem[p[2]];
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
                for (int c = 0; c < 3; ++c) acc[j][c] += kv * (double)deg_tile[c * T * T + at];
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

// ---------------------------------------------------------------- bilinear
struct Tap {
    int i0, i1;
    float a0, a1;
};

IR_DEVINL Tap tap_of(int d, int src, int dst) {
    float f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) s = 0, f = 0.0f;
    if (s >= src - 1) s = src - 1, f = 0.0f;
    return Tap{s, s + 1 < src ? s + 1 : src - 1, 1.0f - f, f};
}

// one pixel of cv2.resize(src [sh][sw][3], (dw, dh), INTER_LINEAR): rows first, then columns
IR_DEVINL void bilinear_px(const float* __restrict__ src, int sh, int sw, int dh, int dw, int dy, int dx, float v[3]) {
    const Tap tx = tap_of(dx, sw, dw), ty = tap_of(dy, sh, dh);
    const float* r0 = src + (long)ty.i0 * sw * 3;
    const float* r1 = src + (long)ty.i1 * sw * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = tx.a0 * r0[3 * tx.i0 + c] + tx.a1 * r0[3 * tx.i1 + c];
        const float bot = tx.a0 * r1[3 * tx.i0 + c] + tx.a1 * r1[3 * tx.i1 + c];
        v[c] = ty.a0 * top + ty.a1 * bot;
    }
}

__global__ __launch_bounds__(TPB) void degrade_down_kernel(const float* __restrict__ src, int h, int w, int lh, int lw, const float* __restrict__ noise,
                                                           float sigma, float* __restrict__ low) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)lh * lw) return;
    const int dy = (int)(i / lw), dx = (int)(i - (long)dy * lw);
    float v[3];
    bilinear_px(src, h, w, lh, lw, dy, dx, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = v[c];
        if (noise) {
            x = x + noise[i * 3 + c] * sigma / 255.0f;
            x = fminf(fmaxf(x, 0.0f), 1.0f);
        }
        low[i * 3 + c] = x;
    }
}

// ---------------------------------------------------------------- JPEG: colour conversion and chroma downsample
struct Ycc {
    int y, cb, cr;
};

IR_DEVINL Ycc ycc_at(const float* __restrict__ low, int lw, int y, int x) {
    const float* p = low + ((long)y * lw + x) * 3;
    const int r = clampi((int)rintf(p[0] * 255.0f), 0, 255), g = clampi((int)rintf(p[1] * 255.0f), 0, 255), b = clampi((int)rintf(p[2] * 255.0f), 0, 255);
    return Ycc{(FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16,
               (-FIX(.16874) * r - FIX(.33126) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16,
               (FIX(.5) * r - FIX(.41869) * g - FIX(.08131) * b + (128 << 16) + 32767) >> 16};
}

// one thread per chroma sample of the padded planes: its 2 x 2 luma samples and its Cb and Cr
__global__ __launch_bounds__(TPB) void degrade_ycc_kernel(const float* __restrict__ low, int lh, int lw, int PH, int PW, uint8_t* __restrict__ Y,
                                                          uint8_t* __restrict__ Cb, uint8_t* __restrict__ Cr) {
    const int CW = PW >> 1, CH = PH >> 1;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= CW * CH) return;
    const int cy = i / CW, cx = i - cy * CW;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int py = 2 * cy + dy, px = 2 * cx + dx;
            Y[py * PW + px] = (uint8_t)ycc_at(low, lw, py < lh ? py : lh - 1, px < lw ? px : lw - 1).y;
        }
    const int ch = (lh + 1) >> 1, sy = cy < ch ? cy : ch - 1;   // rows past the true chroma height repeat the last DOWNSAMPLED row
    const int ya = 2 * sy, yb = 2 * sy + 1 < lh ? 2 * sy + 1 : lh - 1;   // full-resolution rows replicate to an even count only
    const int xa = 2 * cx < lw ? 2 * cx : lw - 1, xb = 2 * cx + 1 < lw ? 2 * cx + 1 : lw - 1;
    const Ycc p0 = ycc_at(low, lw, ya, xa), p1 = ycc_at(low, lw, ya, xb), p2 = ycc_at(low, lw, yb, xa), p3 = ycc_at(low, lw, yb, xb);
    const int bias = 1 + (cx & 1);
    Cb[i] = (uint8_t)((p0.cb + p1.cb + p2.cb + p3.cb + bias) >> 2);
    Cr[i] = (uint8_t)((p0.cr + p1.cr + p2.cr + p3.cr + bias) >> 2);
}

// ---------------------------------------------------------------- JPEG: the DCT round trip of 8 x 8 blocks
struct QTables {
    uint16_t t[2][64];   // luminance, chrominance; natural order
};

template <bool FIRST>
IR_DEVINL void fdct8(i64 d[8]) {   // jfdctint.c, one row (FIRST) or one column
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    i64 t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const i64 t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    i64 z1 = (t12 + t13) * F_0_541;
    d[2] = descale(z1 + t13 * F_0_765, N);
    d[6] = descale(z1 + t12 * (-F_1_847), N);
    z1 = t4 + t7;
    i64 z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const i64 z5 = (z3 + z4) * F_1_175;
    t4 *= F_0_298, t5 *= F_2_053, t6 *= F_3_072, t7 *= F_1_501;
    z1 *= -F_0_899, z2 *= -F_2_562, z3 *= -F_1_961, z4 *= -F_0_390;
    z3 += z5, z4 += z5;
    d[7] = descale(t4 + z1 + z3, N);
    d[5] = descale(t5 + z2 + z4, N);
    d[3] = descale(t6 + z2 + z3, N);
    d[1] = descale(t7 + z1 + z4, N);
}

// planes [gridDim.y][H][W] bytes, H and W multiples of 8; lane l of a group of eight takes row l, column l, column l, row l of its block
__global__ __launch_bounds__(TPB) void degrade_dct_kernel(uint8_t* __restrict__ planes, int H, int W, QTables qt, int table) {
    __shared__ int s_c[TPB / 8][8][9];
    const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
    const int bw = W >> 3, nblk = bw * (H >> 3), blk = blockIdx.x * (TPB / 8) + g;
    const bool live = blk < nblk;
    const int by = live ? blk / bw : 0, bx = live ? blk - by * bw : 0;
    uint8_t* row = planes + (long)blockIdx.y * H * W + (long)(by * 8 + l) * W + bx * 8;
    i64 d[8];
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (int)row[i] - 128;
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_c[g][l][i] = (int)d[i];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_c[g][i][l];
        fdct8<false>(d);   // the coefficients of column l, scaled by 8
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int Q = qt.t[table][i * 8 + l], c = (int)d[i];
            const int m = ((c < 0 ? -c : c) + 4 * Q) / (8 * Q);
            d[i] = (c < 0 ? -m : m) * Q;
        }
        idct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) s_c[g][i][l] = (int)d[i];   // this lane's own column: nobody else reads or writes it in between
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s_c[g][l][i];
        idct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = (uint8_t)clampi((int)d[i] + 128, 0, 255);
    }
}

// ---------------------------------------------------------------- JPEG: fancy upsampling and back to RGB
__global__ __launch_bounds__(TPB) void degrade_rgb_kernel(const uint8_t* __restrict__ Y, const uint8_t* __restrict__ Cb, const uint8_t* __restrict__ Cr,
                                                          int lh, int lw, int PW, float* __restrict__ low, uint8_t* __restrict__ bytes) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= lh * lw) return;
    const int y = i / lw, x = i - y * lw, CW = PW >> 1, ch = (lh + 1) >> 1, cw = (lw + 1) >> 1;
    const int yy = Y[y * PW + x], cb = chroma_up(Cb, CW, ch, cw, y, x) - 128, cr = chroma_up(Cr, CW, ch, cw, y, x) - 128;
    const int rgb[3] = {clampi(yy + ((FIX(1.402) * cr + 32768) >> 16), 0, 255),
                        clampi(yy + ((-FIX(.34414) * cb - FIX(.71414) * cr + 32768) >> 16), 0, 255),
                        clampi(yy + ((FIX(1.772) * cb + 32768) >> 16), 0, 255)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        low[(long)i * 3 + c] = unit(rgb[c]);
        if (bytes) bytes[(long)i * 3 + c] = (uint8_t)rgb[c];
    }
}

// ---------------------------------------------------------------- back to h x w, to bytes
// MAXNORM: keep the floats in `flt` and the maximum of the workgroup's patch in part[workgroup]
template <bool MAXNORM>
__global__ __launch_bounds__(TPB) void degrade_up_kernel(const float* __restrict__ low, int lh, int lw, int h, int w, uint8_t* __restrict__ out,
                                                         long out_pitch, float* __restrict__ flt, float* __restrict__ part) {
    __shared__ float s_max[TPB];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x = blockIdx.x * PATCH + tx;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = blockIdx.y * PATCH + ty + 8 * j;
        if (x < w && y < h) {
            float v[3];
            bilinear_px(low, lh, lw, h, w, y, x, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (MAXNORM) {
                    flt[((long)y * w + x) * 3 + c] = v[c];
                    mx = fmaxf(mx, v[c]);
                } else {
                    out[(long)y * out_pitch + 3 * x + c] = (uint8_t)truncf(fminf(fmaxf(v[c], 0.0f), 1.0f) * 255.0f);
                }
            }
        }
    }
    if constexpr (MAXNORM) {
        s_max[threadIdx.x] = mx;
        __syncthreads();
        for (int o = TPB / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = s_max[0];
    }
}

// one workgroup: part[count] is the maximum of part[0 .. count)
__global__ __launch_bounds__(TPB) void degrade_fold_max_kernel(float* __restrict__ part, int count) {
    __shared__ float s_max[TPB];
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < count; i += TPB) mx = fmaxf(mx, part[i]);
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[count] = s_max[0];
}

__global__ __launch_bounds__(TPB) void degrade_norm_max_kernel(const float* __restrict__ flt, const float* __restrict__ m_at, int h, int w,
                                                               uint8_t* __restrict__ out, long out_pitch) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= (long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long)y * w);
    const float m = *m_at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fmaxf(flt[i * 3 + c], 0.0f);
        out[(long)y * out_pitch + 3 * x + c] = m > 0.0f ? (uint8_t)truncf(v / m * 255.0f) : (uint8_t)0;   // an all-black image stays black
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Layout {
    size_t flt, low, y, cb, cr, part, total;
};

Layout layout(int h, int w) {
    const size_t PH = (size_t)(h + 15) & ~(size_t)15, PW = (size_t)(w + 15) & ~(size_t)15;
    const size_t parts = (size_t)((h + PATCH - 1) / PATCH) * ((w + PATCH - 1) / PATCH);
    Layout l;
    size_t at = 0;
    l.flt = at, at += up256((size_t)h * w * 3 * sizeof(float));
    l.low = at, at += up256((size_t)h * w * 3 * sizeof(float));
    l.y = at, at += up256(PH * PW);
    l.cb = at, at += up256(PH * PW / 4);   // Cb and Cr lie behind each other: one dct launch takes both
    l.cr = at, at += up256(PH * PW / 4);
    l.part = at, at += up256((parts + 1) * sizeof(float));
    l.total = at;
    return l;
}

}  // namespace

void ir_degrade_qtables_host(int q, uint16_t* luma64, uint16_t* chroma64) {
    static const uint8_t base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (base[t][i] * s + 50) / 100;
            (t ? chroma64 : luma64)[i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

size_t ir_degrade_workspace(int h, int w) { return (h < 1 || w < 1) ? 0 : layout(h, w).total; }

int ir_launch_degrade(const uint8_t* img, long pitch, int h, int w, const double* k, int K, int lh, int lw, float sigma, int q, const float* noise,
                      int norm, uint8_t* out, long out_pitch, uint8_t* jpeg, void* ws, hipStream_t s) {
    if (K < 1 || K > IR_DEGRADE_MAX_KSIZE || !(K & 1) || h < K / 2 + 1 || w < K / 2 + 1 || lh < IR_DEGRADE_MIN_LOW || lw < IR_DEGRADE_MIN_LOW ||
        lh > h || lw > w || q < 0 || q > 100 || (long)h * w > (1L << 28))
        return -1;
    const Layout l = layout(h, w);
    uint8_t* base = static_cast<uint8_t*>(ws);
    float* flt = reinterpret_cast<float*>(base + l.flt);
    float* low = reinterpret_cast<float*>(base + l.low);
    float* part = reinterpret_cast<float*>(base + l.part);
    const dim3 patches((w + PATCH - 1) / PATCH, (h + PATCH - 1) / PATCH);
    if (patches.y > 65535) return -1;
    const int T = PATCH + K - 1;
    static_assert((size_t)(PATCH + IR_DEGRADE_MAX_KSIZE - 1) * (PATCH + IR_DEGRADE_MAX_KSIZE - 1) * 12 + 1024 <= 64 * 1024, "the blur's halo tile must fit in LDS");
    hipLaunchKernelGGL(degrade_blur_kernel, patches, dim3(TPB), ((size_t)T * T * 3 + 256) * sizeof(float), s, img, pitch, h, w, k, K, flt);
    const int low_px = lh * lw;
    hipLaunchKernelGGL(degrade_down_kernel, dim3((low_px + TPB - 1) / TPB), dim3(TPB), 0, s, flt, h, w, lh, lw, noise, sigma, low);
    if (q > 0) {
        const int PH = (lh + 15) & ~15, PW = (lw + 15) & ~15;
        uint8_t *Y = base + l.y, *Cb = base + l.cb, *Cr = Cb + (size_t)PH * PW / 4;   // the planes of THIS low size, Cr right behind Cb
        QTables qt;
        ir_degrade_qtables_host(q, qt.t[0], qt.t[1]);
        hipLaunchKernelGGL(degrade_ycc_kernel, dim3((PH * PW / 4 + TPB - 1) / TPB), dim3(TPB), 0, s, low, lh, lw, PH, PW, Y, Cb, Cr);
        constexpr int PER = TPB / 8;
        hipLaunchKernelGGL(degrade_dct_kernel, dim3((PH * PW / 64 + PER - 1) / PER, 1), dim3(TPB), 0, s, Y, PH, PW, qt, 0);
        hipLaunchKernelGGL(degrade_dct_kernel, dim3((PH * PW / 256 + PER - 1) / PER, 2), dim3(TPB), 0, s, Cb, PH / 2, PW / 2, qt, 1);
        hipLaunchKernelGGL(degrade_rgb_kernel, dim3((low_px + TPB - 1) / TPB), dim3(TPB), 0, s, Y, Cb, Cr, lh, lw, PW, low, jpeg);
    }
    if (norm == NORM_MAX) {
        const int parts = (int)(patches.x * patches.y);
        hipLaunchKernelGGL(degrade_up_kernel<true>, patches, dim3(TPB), 0, s, low, lh, lw, h, w, out, out_pitch, flt, part);
        hipLaunchKernelGGL(degrade_fold_max_kernel, dim3(1), dim3(TPB), 0, s, part, parts);
        hipLaunchKernelGGL(degrade_norm_max_kernel, dim3((unsigned)(((long)h * w + TPB - 1) / TPB)), dim3(TPB), 0, s, flt, part + parts, h, w, out,
                           out_pitch);
    } else {
        hipLaunchKernelGGL(degrade_up_kernel<false>, patches, dim3(TPB), 0, s, low, lh, lw, h, w, out, out_pitch, flt, part);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
