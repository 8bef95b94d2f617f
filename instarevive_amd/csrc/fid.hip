// The Inception-v3 features of FID from uint8 HWC RGB device images (ir_fid_features): the model of tools/evaluate_fid.py::InceptionFID, exact fp32
// convolutions and an fp64 tail. The n images of a call go through one set of launches:
//   the resize to 299 x 299 in one kernel, a thread per output pixel. `clean`: Pillow's float BICUBIC - the double coefficient tables come from
//   the host (ir_fid_resize_plan); a thread makes, for every row of its vertical support, the horizontal sum ss += (double)pixel * k in Pillow's
//   order, rounds it to float32 as Pillow stores the image between its passes, and adds the rows in double in the same way; clip to [0, 255],
//   (v - 128) / 128. Nothing is kept between the passes, so the workspace does not depend on the image's size. `legacy`: torch's fp32 bilinear,
//   fmaf(p0, w0, p1 * w1) along x and then along y. The network's input map has four channels, the fourth zero.
//   The 94 convolutions as implicit GEMMs on the exact-fp32 tile loop of exact_f32_tile.h, with what Inception needs: kh x kw
//   kernels with their own paddings, stride 1 or 2, a k-tile that may cross a tap (K = kh kw cin in (ky, kx, c) order, cin a multiple of 4: a
//   thread's float4 of the A tile has its own tap, so cin = 48 and 80 need no padded maps; zero rows behind K and a zero fourth input channel
//   are exact, fmaf(0, 0, acc) = acc), cout padded to the 64-column tile in the weights alone, and an epilogue relu(acc * scale + shift) - the
//   BatchNorm folded in fp64 by ir_fid_configure, product and sum rounded separately (the file is built with -ffp-contract=off) - that writes
//   into a channel slice of a wider NHWC map (pitch + offset), so a block's concatenation costs nothing. The tile is 128 x 64, or 64 x 64
//   where 128-row tiles would leave most of the chip idle (the 8 x 8 and 17 x 17 maps of few images).
//   Pools: 3 x 3, stride 1 (padding 1) or 2 (no padding); max, where padding never wins, or the average over the in-bounds taps, added row by row
//   from the top-left and divided once by their count.
//   Means: a lane per channel, the pixels dealt to the waves of a workgroup, the waves' fp64 sums added in wave order, one division: the 2048
//   features, and on request the per-channel means of thirteen maps.
// Reads are clipped to the scored rectangle h x w; every store is guarded by the row / element count of its launch.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "common.h"
#include "exact_f32_tile.h"
#include "kernels.h"

namespace {

using namespace exact_tile;
constexpr int BN = 64;
constexpr int S = IR_FID_SIZE;
constexpr int MEAN_TPB = 1024;
constexpr int RESIZE_CLEAN = 0;   // IR_FID_RESIZE_CLEAN of the public header

struct ResizeArgs {
    const uint8_t* img;
    long pitch, img_bytes;
    int h, w, kx, ky;
    const int *xb, *yb;        // [299][2]: first tap, taps (clean) / the two source indices (legacy)
    const double *xk, *yk;     // [299][kx], [299][ky]
    const float* x01;          // [256] (float)v / 255.0f
    float* x4;                 // [n][299][299][4]
    float* resized;            // [n][299][299][3] or null
    long total;                // n * 299 * 299
};

__global__ __launch_bounds__(TPB) void fid_resize_clean_kernel(ResizeArgs p) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= p.total) return;
    const int ox = (int)(i % S);
    const long r = i / S;
    const int oy = (int)(r % S);
    const uint8_t* img = p.img + (r / S) * p.img_bytes;
    const int x0 = p.xb[2 * ox], xn = min(p.xb[2 * ox + 1], p.kx), y0 = p.yb[2 * oy], yn = min(p.yb[2 * oy + 1], p.ky);
    const double* xk = p.xk + (long)ox * p.kx;
    const double* yk = p.yk + (long)oy * p.ky;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int y = 0; y < yn; ++y) {
        const uint8_t* row = img + (long)min(max(y0 + y, 0), p.h - 1) * p.pitch;
        double ss[3] = {0.0, 0.0, 0.0};
        for (int x = 0; x < xn; ++x) {
            const uint8_t* px = row + 3L * min(max(x0 + x, 0), p.w - 1);
            const double k = xk[x];
#pragma unroll
            for (int c = 0; c < 3; ++c) ss[c] = ss[c] + (double)(float)px[c] * k;
        }
        const double k = yk[y];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (double)(float)ss[c] * k;
    }
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fminf(fmaxf((float)acc[c], 0.f), 255.f);
    if (p.resized) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.resized[3 * i + c] = v[c];
    }
    reinterpret_cast<float4*>(p.x4)[i] = make_float4((v[0] - 128.f) / 128.f, (v[1] - 128.f) / 128.f, (v[2] - 128.f) / 128.f, 0.f);
}

__global__ __launch_bounds__(TPB) void fid_resize_legacy_kernel(ResizeArgs p) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= p.total) return;
    const int ox = (int)(i % S);
    const long r = i / S;
    const int oy = (int)(r % S);
    const uint8_t* img = p.img + (r / S) * p.img_bytes;
    const int xi[2] = {min(max(p.xb[2 * ox], 0), p.w - 1), min(max(p.xb[2 * ox + 1], 0), p.w - 1)};
    const float wx0 = (float)p.xk[2 * ox], wx1 = (float)p.xk[2 * ox + 1], wy0 = (float)p.yk[2 * oy], wy1 = (float)p.yk[2 * oy + 1];
    const uint8_t* r0 = img + (long)min(max(p.yb[2 * oy], 0), p.h - 1) * p.pitch;
    const uint8_t* r1 = img + (long)min(max(p.yb[2 * oy + 1], 0), p.h - 1) * p.pitch;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t0 = fmaf(p.x01[r0[3 * xi[0] + c]], wx0, p.x01[r0[3 * xi[1] + c]] * wx1);
        const float t1 = fmaf(p.x01[r1[3 * xi[0] + c]], wx0, p.x01[r1[3 * xi[1] + c]] * wx1);
        v[c] = fmaf(t0, wy0, t1 * wy1);
    }
    if (p.resized) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.resized[3 * i + c] = v[c];
    }
    reinterpret_cast<float4*>(p.x4)[i] = make_float4(2.f * v[0] - 1.f, 2.f * v[1] - 1.f, 2.f * v[2] - 1.f, 0.f);
}

struct ConvArgs {
    const float* in;            // [imgs][H][W][in_pitch], the first cin channels
    int in_pitch, H, W, cin;    // cin: a multiple of 4
    int kh, kw, stride, ph, pw;
    int Ho, Wo;
    int M, K, N, Npad;          // M = imgs * Ho * Wo, K = kh * kw * cin (un-padded), N = cout, Npad = N rounded up to 64
    const float* wgt;           // [K rounded up to 32][Npad]
    const float *scale, *shift; // [N]
    float* out;                 // [M][out_pitch], channels out_off .. out_off + N - 1
    int out_pitch, out_off;
};

// BatchNorm (scale, shift) and ReLU into the channel slice
struct BnRelu {
    const ConvArgs& p;
    int col;
    float sc, sh;
    IR_DEVINL bool column(int c) {
        if (c >= p.N) return false;   // cout is padded to the tile in the weights alone
        col = c;
        sc = p.scale[c];
        sh = p.shift[c];
        return true;
    }
    IR_DEVINL void store(int m, float acc) const { p.out[(long)m * p.out_pitch + p.out_off + col] = fmaxf(acc * sc + sh, 0.f); }
};

template <int BM>
__global__ __launch_bounds__(TPB, BM == 64 ? 7 : 4) void fid_conv_kernel(ConvArgs p) {
    const NhwcA<BM, false> a{.in = p.in, .H = p.H, .W = p.W, .cin = p.cin, .pitch = p.in_pitch, .kw = p.kw, .stride = p.stride, .ph = p.ph, .pw = p.pw, .Ho = p.Ho, .Wo = p.Wo, .M = p.M, .K = p.K};
    const KnB<BN, false> b{.b = p.wgt, .ldb = p.Npad};
    tile_loop<BM, BN>(a, b, p.M, p.K, BnRelu{p});
}

struct PoolArgs {
    const float* in;   // [imgs][H][W][in_pitch], the first 4 * C4 channels
    float* out;        // [imgs][Ho][Wo][out_pitch], channels out_off ..
    int in_pitch, out_pitch, out_off;
    int H, W, C4, Ho, Wo, stride, pad;
    long total;        // imgs * Ho * Wo * C4
};

// a thread per four channels of an output pixel; AVG: the mean of the in-bounds taps, else their maximum
template <bool AVG>
__global__ __launch_bounds__(TPB) void fid_pool_kernel(PoolArgs p) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= p.total) return;
    const int c = (int)(i % p.C4);
    long r = i / p.C4;
    const long pix = r;
    const int ox = (int)(r % p.Wo);
    r /= p.Wo;
    const int oy = (int)(r % p.Ho);
    const long img = r / p.Ho;
    const float inf = __builtin_huge_valf();
    float4 s = AVG ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-inf, -inf, -inf, -inf);
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * p.stride - p.pad + dy;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * p.stride - p.pad + dx;
            if (iy < 0 || iy >= p.H || ix < 0 || ix >= p.W) continue;
            const float4 v = *reinterpret_cast<const float4*>(p.in + ((img * p.H + iy) * p.W + ix) * p.in_pitch + 4 * c);
            ++cnt;
            if constexpr (AVG) {
                s.x = s.x + v.x;
                s.y = s.y + v.y;
                s.z = s.z + v.z;
                s.w = s.w + v.w;
            } else {
                s.x = fmaxf(s.x, v.x);
                s.y = fmaxf(s.y, v.y);
                s.z = fmaxf(s.z, v.z);
                s.w = fmaxf(s.w, v.w);
            }
        }
    }
    if constexpr (AVG) {
        const float d = (float)max(cnt, 1);
        s = make_float4(__fdiv_rn(s.x, d), __fdiv_rn(s.y, d), __fdiv_rn(s.z, d), __fdiv_rn(s.w, d));
    }
    *reinterpret_cast<float4*>(p.out + pix * p.out_pitch + p.out_off + 4 * c) = s;
}

// map: [imgs][HW][C]; workgroup (x, img): channels 64 x .. 64 x + 63, a lane per channel, pixel q on wave q % 16;
// out[img * out_stride + out_off + c] = the mean in fp64
__global__ __launch_bounds__(MEAN_TPB) void fid_mean_kernel(const float* __restrict__ map, int HW, int C, double* __restrict__ out, long out_stride, int out_off) {
    constexpr int WAVES = MEAN_TPB / 64;
    __shared__ double s_red[WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const long img = blockIdx.y;
    double s = 0.0;
    if (c < C) {
        const float* f = map + img * HW * C + c;
        for (int q = wave; q < HW; q += WAVES) s += (double)f[(long)q * C];
    }
    s_red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < C) {
        double v = s_red[0][lane];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) v += s_red[k][lane];
        out[img * out_stride + out_off + c] = v / (double)HW;
    }
}

struct Flow {
    const IrFidModel& m;
    int n;
    hipStream_t s;
    int conv = 0;   // the next convolution of ir_fid_convs()
    bool bad = false;   // a launch that would leave its buffers was skipped (cannot happen with the flow below)

    // the conv reads the first cin channels of `in` (pitch floats per pixel) and writes channels off .. of `out`; returns its output edge
    int run_conv(const float* in, int in_pitch, int H, float* out, int out_pitch, int off) {
        if (conv >= IR_FID_CONVS) {
            bad = true;
            return H;
        }
        const IrFidConv& c = ir_fid_convs()[conv];
        ConvArgs p{};
        p.in = in; p.in_pitch = in_pitch; p.H = p.W = H; p.cin = c.cin == 3 ? 4 : c.cin;
        p.kh = c.kh; p.kw = c.kw; p.stride = c.stride; p.ph = c.ph; p.pw = c.pw;
        p.Ho = (H + 2 * c.ph - c.kh) / c.stride + 1;
        p.Wo = (H + 2 * c.pw - c.kw) / c.stride + 1;
        p.M = n * p.Ho * p.Wo; p.K = c.kh * c.kw * p.cin; p.N = c.cout; p.Npad = (c.cout + BN - 1) / BN * BN;
        p.wgt = m.w[conv]; p.scale = m.scale[conv]; p.shift = m.shift[conv];
        p.out = out; p.out_pitch = out_pitch; p.out_off = off;
        const unsigned gn = (unsigned)(p.Npad / BN);
        if (p.cin > in_pitch || (in_pitch & 3) || off + c.cout > out_pitch || (long)p.Ho * p.Wo * out_pitch > IR_FID_MAP_FLOATS) {
            bad = true;
            ++conv;
            return p.Ho;
        }
        if ((long)((p.M + 127) / 128) * gn >= 256)
            hipLaunchKernelGGL((fid_conv_kernel<128>), dim3((unsigned)((p.M + 127) / 128), gn), dim3(TPB), 0, s, p);
        else
            hipLaunchKernelGGL((fid_conv_kernel<64>), dim3((unsigned)((p.M + 63) / 64), gn), dim3(TPB), 0, s, p);
        ++conv;
        return p.Ho;
    }
    int pool(bool avg, const float* in, int C, int H, int stride, int pad, float* out, int out_pitch, int off) {
        PoolArgs p{};
        p.in = in; p.out = out; p.in_pitch = C; p.out_pitch = out_pitch; p.out_off = off;
        p.H = p.W = H; p.C4 = C / 4; p.Ho = p.Wo = (H + 2 * pad - 3) / stride + 1; p.stride = stride; p.pad = pad;
        p.total = (long)n * p.Ho * p.Wo * p.C4;
        if ((C & 3) || (out_pitch & 3) || (off & 3) || off + C > out_pitch || (long)p.Ho * p.Wo * out_pitch > IR_FID_MAP_FLOATS) {
            bad = true;
            return p.Ho;
        }
        const dim3 grid((unsigned)((p.total + TPB - 1) / TPB));
        if (avg)
            hipLaunchKernelGGL(fid_pool_kernel<true>, grid, dim3(TPB), 0, s, p);
        else
            hipLaunchKernelGGL(fid_pool_kernel<false>, grid, dim3(TPB), 0, s, p);
        return p.Ho;
    }
    void mean(const float* map, int H, int C, double* out, long stride, int off) {
        hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)n), dim3(MEAN_TPB), 0, s, map, H * H, C, out, stride, off);
    }
};

}  // namespace

namespace {

std::vector<IrFidConv> make_fid_convs() {
    std::vector<IrFidConv> v;
    auto add = [&](const std::string& name, int cin, int cout, int kh = 1, int kw = 1, int stride = 1, int ph = 0, int pw = 0) {
        IrFidConv c{};
        snprintf(c.name, sizeof c.name, "%s", name.c_str());
        c.cin = cin; c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride; c.ph = ph; c.pw = pw;
        v.push_back(c);
    };
    add("Conv2d_1a_3x3", 3, 32, 3, 3, 2);
    add("Conv2d_2a_3x3", 32, 32, 3, 3);
    add("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
    add("Conv2d_3b_1x1", 64, 80);
    add("Conv2d_4a_3x3", 80, 192, 3, 3);
    auto block_a = [&](const std::string& b, int cin, int pf) {
        add(b + ".branch1x1", cin, 64);
        add(b + ".branch5x5_1", cin, 48);
        add(b + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
        add(b + ".branch3x3dbl_1", cin, 64);
        add(b + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
        add(b + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
        add(b + ".branch_pool", cin, pf);
    };
    auto block_c = [&](const std::string& b, int c7) {
        add(b + ".branch1x1", 768, 192);
        add(b + ".branch7x7_1", 768, c7);
        add(b + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3);
        add(b + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0);
        add(b + ".branch7x7dbl_1", 768, c7);
        add(b + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0);
        add(b + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3);
        add(b + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0);
        add(b + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3);
        add(b + ".branch_pool", 768, 192);
    };
    auto block_e = [&](const std::string& b, int cin) {
        add(b + ".branch1x1", cin, 320);
        add(b + ".branch3x3_1", cin, 384);
        add(b + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
        add(b + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
        add(b + ".branch3x3dbl_1", cin, 448);
        add(b + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
        add(b + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
        add(b + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
        add(b + ".branch_pool", cin, 192);
    };
    block_a("Mixed_5b", 192, 32);
    block_a("Mixed_5c", 256, 64);
    block_a("Mixed_5d", 288, 64);
    add("Mixed_6a.branch3x3", 288, 384, 3, 3, 2);
    add("Mixed_6a.branch3x3dbl_1", 288, 64);
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2);
    block_c("Mixed_6b", 128);
    block_c("Mixed_6c", 160);
    block_c("Mixed_6d", 160);
    block_c("Mixed_6e", 192);
    add("Mixed_7a.branch3x3_1", 768, 192);
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2);
    add("Mixed_7a.branch7x7x3_1", 768, 192);
    add("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
    add("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2);
    block_e("Mixed_7b", 1280);
    block_e("Mixed_7c", 2048);
    return v;
}

}  // namespace

const IrFidConv* ir_fid_convs() {
    static const std::vector<IrFidConv> t = make_fid_convs();   // initialised once, also under concurrent first calls
    return t.data();
}

int ir_fid_plan(int n, IrFidPlan* pl) {
    if (n < 1 || n > IR_FID_MAX_N) return -1;
    pl->x4_bytes = ((size_t)n * S * S * 4 * sizeof(float) + 255) & ~(size_t)255;
    pl->map_bytes = ((size_t)n * IR_FID_MAP_FLOATS * sizeof(float) + 255) & ~(size_t)255;
    pl->total = pl->x4_bytes + 4 * pl->map_bytes;
    return 0;
}

int ir_launch_fid(const IrFidModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, int mode, const void* tables, double* features,
                  double* block_means, float* resized, void* ws, hipStream_t s) {
    IrFidPlan pl;
    IrFidTables tl;
    if (ir_fid_plan(n, &pl) || ir_fid_tables_layout(h, w, mode, &tl)) return -1;
    char* base = static_cast<char*>(ws);
    float* x4 = reinterpret_cast<float*>(base);
    float* cur = reinterpret_cast<float*>(base + pl.x4_bytes);
    float* oth = reinterpret_cast<float*>(base + pl.x4_bytes + pl.map_bytes);
    float* t1 = reinterpret_cast<float*>(base + pl.x4_bytes + 2 * pl.map_bytes);
    float* t2 = reinterpret_cast<float*>(base + pl.x4_bytes + 3 * pl.map_bytes);

    const char* tb = static_cast<const char*>(tables);
    ResizeArgs ra{};
    ra.img = img; ra.pitch = pitch; ra.img_bytes = (long)rows * pitch; ra.h = h; ra.w = w; ra.kx = tl.kx; ra.ky = tl.ky;
    ra.xb = reinterpret_cast<const int*>(tb + tl.xb); ra.yb = reinterpret_cast<const int*>(tb + tl.yb);
    ra.xk = reinterpret_cast<const double*>(tb + tl.xk); ra.yk = reinterpret_cast<const double*>(tb + tl.yk);
    ra.x01 = m.x01; ra.x4 = x4; ra.resized = resized; ra.total = (long)n * S * S;
    const dim3 rgrid((unsigned)((ra.total + TPB - 1) / TPB));
    if (mode == RESIZE_CLEAN)
        hipLaunchKernelGGL(fid_resize_clean_kernel, rgrid, dim3(TPB), 0, s, ra);
    else
        hipLaunchKernelGGL(fid_resize_legacy_kernel, rgrid, dim3(TPB), 0, s, ra);

    Flow f{m, n, s};
    int blk = 0, off = 0;
    auto means = [&](const float* map, int H, int C) {   // the next of the thirteen maps of block_means
        if (block_means) f.mean(map, H, C, block_means, IR_FID_BLOCK_CHANNELS, off);
        off += C;
        ++blk;
    };
    int H = f.run_conv(x4, 4, S, cur, 32, 0);           // 149
    H = f.run_conv(cur, 32, H, oth, 32, 0);             // 147
    H = f.run_conv(oth, 32, H, cur, 64, 0);
    means(cur, H, 64);
    H = f.pool(false, cur, 64, H, 2, 0, oth, 64, 0);    // 73
    H = f.run_conv(oth, 64, H, cur, 80, 0);
    H = f.run_conv(cur, 80, H, oth, 192, 0);            // 71
    means(oth, H, 192);
    H = f.pool(false, oth, 192, H, 2, 0, cur, 192, 0);  // 35
    int C = 192;
    for (int k = 0; k < 3; ++k) {   // Mixed_5b / 5c / 5d
        const int pf = k == 0 ? 32 : 64, Co = 224 + pf;
        f.run_conv(cur, C, H, oth, Co, 0);
        f.run_conv(cur, C, H, t1, 48, 0);
        f.run_conv(t1, 48, H, oth, Co, 64);
        f.run_conv(cur, C, H, t1, 64, 0);
        f.run_conv(t1, 64, H, t2, 96, 0);
        f.run_conv(t2, 96, H, oth, Co, 128);
        f.pool(true, cur, C, H, 1, 1, t1, C, 0);
        f.run_conv(t1, C, H, oth, Co, 224);
        std::swap(cur, oth);
        C = Co;
        means(cur, H, C);
    }
    {   // Mixed_6a: 35 -> 17, 288 -> 768
        f.run_conv(cur, C, H, oth, 768, 0);
        f.run_conv(cur, C, H, t1, 64, 0);
        f.run_conv(t1, 64, H, t2, 96, 0);
        f.run_conv(t2, 96, H, oth, 768, 384);
        H = f.pool(false, cur, C, H, 2, 0, oth, 768, 480);
        std::swap(cur, oth);
        C = 768;
        means(cur, H, C);
    }
    for (int k = 0; k < 4; ++k) {   // Mixed_6b .. 6e
        const int c7 = k == 0 ? 128 : k == 3 ? 192 : 160;
        f.run_conv(cur, C, H, oth, 768, 0);
        f.run_conv(cur, C, H, t1, c7, 0);
        f.run_conv(t1, c7, H, t2, c7, 0);
        f.run_conv(t2, c7, H, oth, 768, 192);
        f.run_conv(cur, C, H, t1, c7, 0);
        f.run_conv(t1, c7, H, t2, c7, 0);
        f.run_conv(t2, c7, H, t1, c7, 0);
        f.run_conv(t1, c7, H, t2, c7, 0);
        f.run_conv(t2, c7, H, oth, 768, 384);
        f.pool(true, cur, C, H, 1, 1, t1, C, 0);
        f.run_conv(t1, C, H, oth, 768, 576);
        std::swap(cur, oth);
        means(cur, H, C);
    }
    {   // Mixed_7a: 17 -> 8, 768 -> 1280
        f.run_conv(cur, C, H, t1, 192, 0);
        f.run_conv(t1, 192, H, oth, 1280, 0);
        f.run_conv(cur, C, H, t1, 192, 0);
        f.run_conv(t1, 192, H, t2, 192, 0);
        f.run_conv(t2, 192, H, t1, 192, 0);
        f.run_conv(t1, 192, H, oth, 1280, 320);
        H = f.pool(false, cur, C, H, 2, 0, oth, 1280, 512);
        std::swap(cur, oth);
        C = 1280;
        means(cur, H, C);
    }
    for (int k = 0; k < 2; ++k) {   // Mixed_7b (average pool), Mixed_7c (max pool)
        f.run_conv(cur, C, H, oth, 2048, 0);
        f.run_conv(cur, C, H, t1, 384, 0);
        f.run_conv(t1, 384, H, oth, 2048, 320);
        f.run_conv(t1, 384, H, oth, 2048, 704);
        f.run_conv(cur, C, H, t1, 448, 0);
        f.run_conv(t1, 448, H, t2, 384, 0);
        f.run_conv(t2, 384, H, oth, 2048, 1088);
        f.run_conv(t2, 384, H, oth, 2048, 1472);
        f.pool(k == 0, cur, C, H, 1, 1, t1, C, 0);
        f.run_conv(t1, C, H, oth, 2048, 1856);
        std::swap(cur, oth);
        C = 2048;
        means(cur, H, C);
    }
    if (f.bad || f.conv != IR_FID_CONVS || blk != IR_FID_BLOCKS || off != IR_FID_BLOCK_CHANNELS || H != 8) return -1;
    f.mean(cur, H, C, features, IR_FID_DIM, 0);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
