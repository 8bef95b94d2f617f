// The image tools of the C ABI: PNG and JPEG encoding, Pillow's resampling, PSNR-Y / SSIM-Y, LPIPS, DISTS, FID's features, CLIP-IQA, MUSIQ, MANIQA, TOPIQ-NR, NIQE, IL-NIQE's DFT and Weibull fit and the two degradation paths. Each entry
// point checks its arguments and launches the kernels of its own .hip file; none of them runs a model stage, takes the workspace arena or is
// profiled, so nothing here knows api.cpp's Run. Host code only, except for the tables the kernels read, which are computed here once.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <memory>

#include "host.h"

using namespace ir_host;

namespace {

// ---------------------------------------------------------------- the argument checks the entry points share
// Each returns 0, or -1 with ir_last_error in the words of the entry point `who`. An entry point calls them in its own order.
struct Plane {   // an operand: the rows of each image's slot and the bytes from row to row
    int rows;
    long pitch;
};
// n images of h x w, no edge below min_edge, inside every operand. `tail` says what the minimum is for (null: nothing to say); `also_bad` is the
// entry point's own limit on the same sizes.
int check_rect(ir_ctx* c, const char* who, const char* tail, int n, int h, int w, int min_edge, std::initializer_list<Plane> planes, bool also_bad = false) {
    bool bad = also_bad || n < 1 || h < min_edge || w < min_edge;
    for (const Plane& p : planes) bad |= h > p.rows || p.pitch < 3L * w;
    if (!bad) return 0;
    std::string in;
    for (const Plane& p : planes) in += fmt("%s%d rows pitch %ld", in.empty() ? "" : " and ", p.rows, p.pitch);
    return fail(c, -1, "%s: bad size (n %d, %d x %d in %s%s%s)", who, n, h, w, in.c_str(), tail ? "; " : "", tail ? tail : "");
}
int check_ws(ir_ctx* c, const char* who, const void* ws, size_t ws_bytes, size_t need, uintptr_t align) {
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & (align - 1)))
        return fail(c, -1, "%s: workspace too small or unaligned (%zu < %zu)", who, ws_bytes, need);
    return 0;
}
int check_out8(ir_ctx* c, const char* who, const void* out) {
    if (reinterpret_cast<uintptr_t>(out) & 7) return fail(c, -1, "%s: out not aligned to 8 bytes", who);
    return 0;
}

// ---------------------------------------------------------------- what the LPIPS and CLIP-IQA bindings share
// the tensor `name` of the context with exactly `floats` fp32 values, or null (the caller returns -2) with ir_last_error naming it and `whose` size it misses
const float* exact_f32(ir_ctx* c, const char* who, const char* whose, const std::string& name, size_t floats) {
    auto it = c->t.find(name);
    if (it == c->t.end()) {
        fail(c, -2, "%s: tensor %s (missing)", who, name.c_str());
        return nullptr;
    }
    if (it->second.bytes != floats * 4) {
        fail(c, -2, "%s: tensor %s has %zu bytes, %s has %zu", who, name.c_str(), it->second.bytes, whose, floats * 4);
        return nullptr;
    }
    return static_cast<const float*>(it->second.p);
}
// a conv's device weights [cout][cin][ky][kx] as the host array [(ky, kx, c) padded to 32][cout], zero rows behind K
int repacked_conv(ir_ctx* c, const float* dev_w, int cin, int cout, int ks, std::vector<float>& t) {
    const int K = ks * ks * cin;
    std::vector<float> w((size_t)cout * K);
    HIPOK(c, hipMemcpy(w.data(), dev_w, w.size() * 4, hipMemcpyDeviceToHost));
    t.assign((size_t)pad32(K) * cout, 0.f);
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int ky = 0; ky < ks; ++ky)
                for (int kx = 0; kx < ks; ++kx)
                    t[(size_t)((ky * ks + kx) * cin + ci) * cout + o] = w[(((size_t)o * cin + ci) * ks + ky) * ks + kx];
    return 0;
}
// *out = a copy of `bytes` host or device bytes that `list`, a binding's list of ir_ctx::own, owns
int own_copy(ir_ctx* c, std::vector<void*>& list, const void* src, size_t bytes, hipMemcpyKind kind, const float** out) {
    void* d = nullptr;
    if (dev_alloc(c, list, &d, bytes)) return -100;
    HIPOK(c, hipMemcpy(d, src, bytes, kind));
    *out = static_cast<const float*>(d);
    return 0;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- PNG encoding (png_encode.hip)
// Bytes of one chunk of `rows` rows at most: the 1106-bit block header, at most 9 bits per filtered byte and for the end-of-block symbol (the
// coder never exceeds the fixed 8 / 9-bit code, see png_codes_kernel), 3 bits of the empty stored block's header, the pad to the byte and its
// four LEN / NLEN bytes.
static size_t png_chunk_bound(size_t rows, size_t rowlen) { return (IR_PNG_HEADER_BITS + 9 * (rows * rowlen + 1) + 3 + 7) / 8 + 4; }
struct PngLayout {
    size_t chunks, slot_cap, hist, codes, header, sizes, slots, total;
};
static PngLayout png_layout(int n, int vh, int vw) {
    PngLayout L;
    L.chunks = ((size_t)vh + IR_PNG_ROWS - 1) / IR_PNG_ROWS;
    // a slot is stored in whole 16-byte units and the compaction reads one dword beyond the chunk's last
    L.slot_cap = ((png_chunk_bound(IR_PNG_ROWS, 3 * (size_t)vw + 1) + 15) & ~(size_t)15) + 16;
    const size_t k = (size_t)n * L.chunks;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    L.hist = 0;
    L.codes = L.hist + up(k * 260 * 4);
    L.header = L.codes + up(k * 260 * 4);
    L.sizes = L.header + up(k * 40 * 4);
    L.slots = L.sizes + up(k * 4);
    L.total = L.slots + up(k * L.slot_cap);
    return L;
}
// 2 header bytes + the chunks + 4 bytes of Adler-32. With D = h * (3 w + 1) filtered bytes in ceil(h / IR_PNG_ROWS) chunks the chunk bounds sum
// to at most ceil(9 D / 8) + chunks * (ceil((1106 + 9 + 3 + 7) / 8) + 4 + 1) (the + 1: each chunk's own rounding of 9 * bytes / 8).
size_t ir_png_bound(int h, int w) {
    if (h < 1 || w < 1) return 0;
    const size_t rowlen = 3 * (size_t)w + 1, chunks = ((size_t)h + IR_PNG_ROWS - 1) / IR_PNG_ROWS;
    return 2 + (9 * (size_t)h * rowlen + 7) / 8 + chunks * ((IR_PNG_HEADER_BITS + 9 + 3 + 7 + 7) / 8 + 4 + 1) + 4;
}
int ir_png_encode(ir_ctx* c, void* stream, const uint8_t* img, int n, int h, int w, long pitch, int vh, int vw, uint8_t* out, size_t out_stride,
                  uint32_t* info, void* ws, size_t ws_bytes) {
    if (!c || !img || !out || !info || !ws) return fail(c, -1, "ir_png_encode: null argument");
    if (n < 1 || h < 1 || w < 1 || vh < 1 || vh > h || vw < 1 || vw > w || pitch < 3L * w)
        return fail(c, -1, "ir_png_encode: bad size (n %d, %d x %d, pitch %ld, valid %d x %d)", n, h, w, pitch, vh, vw);
    if (out_stride < ir_png_bound(vh, vw)) return fail(c, -1, "ir_png_encode: out_stride %zu below ir_png_bound(%d, %d) = %zu", out_stride, vh, vw, ir_png_bound(vh, vw));
    const PngLayout L = png_layout(n, vh, vw);
    if (int e = check_ws(c, "ir_png_encode", ws, ws_bytes, L.total, 16)) return e;
    use_ctx(c);
    char* b = static_cast<char*>(ws);
    if (ir_launch_png_encode(img, n, h, pitch, vh, vw, out, out_stride, info, (uint32_t*)(b + L.hist), (uint32_t*)(b + L.codes), (uint32_t*)(b + L.header),
                             (uint32_t*)(b + L.sizes), (uint8_t*)(b + L.slots), (long)L.slot_cap, (hipStream_t)stream))
        return fail(c, -100, "ir_png_encode: launch failed");
    return 0;
}
// The run mode: ir_png_encode's workspace, and behind it per chunk the second histogram, the second code, the second header and the run marks.
struct PngRunsLayout {
    PngLayout lit;
    size_t flag_words, run_hist, run_codes, run_header, flags, total;
};
static PngRunsLayout png_runs_layout(int n, int vh, int vw) {
    PngRunsLayout R;
    R.lit = png_layout(n, vh, vw);
    const size_t k = (size_t)n * R.lit.chunks;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    R.flag_words = ir_png_runs_flag_words(IR_PNG_ROWS * (3 * (size_t)vw + 1));
    R.run_hist = R.lit.total;
    R.run_codes = R.run_hist + up(k * IR_PNG_RUNS_SYMS * 4);
    R.run_header = R.run_codes + up(k * IR_PNG_RUNS_SYMS * 4);
    R.flags = R.run_header + up(k * IR_PNG_RUNS_HEADER_WORDS * 4);
    R.total = R.flags + up(k * R.flag_words * 4);
    return R;
}
int ir_png_encode_runs(ir_ctx* c, void* stream, const uint8_t* img, int n, int h, int w, long pitch, int vh, int vw, uint8_t* out, size_t out_stride,
                       uint32_t* info, void* ws, size_t ws_bytes) {
    if (!c || !img || !out || !info || !ws) return fail(c, -1, "ir_png_encode_runs: null argument");
    if (n < 1 || h < 1 || w < 1 || vh < 1 || vh > h || vw < 1 || vw > w || pitch < 3L * w)
        return fail(c, -1, "ir_png_encode_runs: bad size (n %d, %d x %d, pitch %ld, valid %d x %d)", n, h, w, pitch, vh, vw);
    if (out_stride < ir_png_bound(vh, vw))
        return fail(c, -1, "ir_png_encode_runs: out_stride %zu below ir_png_bound(%d, %d) = %zu", out_stride, vh, vw, ir_png_bound(vh, vw));
    const PngRunsLayout R = png_runs_layout(n, vh, vw);
    const PngLayout& L = R.lit;
    if (int e = check_ws(c, "ir_png_encode_runs", ws, ws_bytes, R.total, 16)) return e;
    use_ctx(c);
    char* b = static_cast<char*>(ws);
    if (ir_launch_png_encode_runs(img, n, h, pitch, vh, vw, out, out_stride, info, (uint32_t*)(b + L.hist), (uint32_t*)(b + L.codes), (uint32_t*)(b + L.header),
                                  (uint32_t*)(b + L.sizes), (uint8_t*)(b + L.slots), (long)L.slot_cap, (uint32_t*)(b + R.run_hist), (uint32_t*)(b + R.run_codes),
                                  (uint32_t*)(b + R.run_header), (uint32_t*)(b + R.flags), (long)R.flag_words, (hipStream_t)stream))
        return fail(c, -100, "ir_png_encode_runs: launch failed");
    return 0;
}

// ---------------------------------------------------------------- JPEG encoding (jpeg_encode.hip)
size_t ir_jpeg_bound(int h, int w, int subsampling, int restart_mcus) { return ir_jpeg_bound_host(h, w, subsampling, restart_mcus); }
int ir_jpeg_encode(ir_ctx* c, void* stream, const uint8_t* img, int n, int h, int w, long pitch, int vh, int vw, int quality, int subsampling,
                   int restart_mcus, uint8_t* out, size_t out_stride, uint32_t* info, void* ws, size_t ws_bytes) {
    if (!c || !img || !out || !info || !ws) return fail(c, -1, "ir_jpeg_encode: null argument");
    if (int e = check_rect(c, "ir_jpeg_encode", nullptr, n, vh, vw, 1, {{h, pitch}}, h < 1 || w < 1 || vw > w || pitch < 3L * w)) return e;
    if (quality < 1 || quality > 100) return fail(c, -1, "ir_jpeg_encode: quality %d outside 1 .. 100", quality);
    if (subsampling != 0 && subsampling != 2) return fail(c, -1, "ir_jpeg_encode: subsampling %d is neither 0 (4:4:4) nor 2 (4:2:0)", subsampling);
    if (restart_mcus < 1 || restart_mcus > 65535) return fail(c, -1, "ir_jpeg_encode: restart interval %d outside 1 .. 65535 MCUs", restart_mcus);
    IrJpegLayout L;
    if (!ir_jpeg_layout(n, vh, vw, subsampling, restart_mcus, &L))
        return fail(c, -1, "ir_jpeg_encode: n %d of %d x %d is more than one call takes (sides and images up to 65535, 2^32 - 1 bytes per image)", n, vh, vw);
    const size_t bound = ir_jpeg_bound_host(vh, vw, subsampling, restart_mcus);
    if (out_stride < bound) return fail(c, -1, "ir_jpeg_encode: out_stride %zu below ir_jpeg_bound(%d, %d, %d, %d) = %zu", out_stride, vh, vw, subsampling, restart_mcus, bound);
    if (int e = check_ws(c, "ir_jpeg_encode", ws, ws_bytes, L.total, 16)) return e;
    use_ctx(c);
    if (ir_launch_jpeg_encode(img, n, h, pitch, vh, vw, quality, subsampling, restart_mcus, out, out_stride, info, ws, (hipStream_t)stream))
        return fail(c, -100, "ir_jpeg_encode: launch failed");
    return 0;
}

// ---------------------------------------------------------------- JPEG decoding (jpeg_decode.hip)
int ir_jpeg_decode(ir_ctx* c, void* stream, const ir_jpeg_file* files, int n, int subseq_bits, uint32_t* info, int16_t* coef_or_null, void* ws,
                   size_t ws_bytes) {
    if (!c || !files || !info || !ws) return fail(c, -1, "ir_jpeg_decode: null argument");
    if (n < 1) return fail(c, -1, "ir_jpeg_decode: n %d", n);
    if (subseq_bits < 128 || subseq_bits > 4096 || subseq_bits % 32) return fail(c, -1, "ir_jpeg_decode: subseq_bits %d is no multiple of 32 in 128 .. 4096", subseq_bits);
    if ((reinterpret_cast<uintptr_t>(info) & 3) || (reinterpret_cast<uintptr_t>(coef_or_null) & 1)) return fail(c, -1, "ir_jpeg_decode: misaligned info or coef pointer");
    size_t need = 0;
    for (int i = 0; i < n; ++i) {   // every file is checked before the first launch
        const char* why;
        if (ir_jpeg_decode_check(&files[i], &why)) return fail(c, -1, "ir_jpeg_decode: file %d (%d x %d): %s", i, files[i].h, files[i].w, why);
        need = std::max(need, ir_jpeg_decode_workspace(files[i].h, files[i].w, files[i].stream_bytes, subseq_bits));
    }
    if (int e = check_ws(c, "ir_jpeg_decode", ws, ws_bytes, need, 256)) return e;
    use_ctx(c);
    for (int i = 0; i < n; ++i) {
        if (ir_launch_jpeg_decode(&files[i], subseq_bits, info + i, coef_or_null, ws, (hipStream_t)stream))
            return fail(c, -100, "ir_jpeg_decode: launch failed (file %d)", i);
        if (coef_or_null) coef_or_null += ir_jpeg_decode_blocks(&files[i]) * 64;
    }
    return 0;
}

// ---------------------------------------------------------------- PNG decoding (png_decode.hip)
int ir_png_decode(ir_ctx* c, void* stream, const ir_png_file* files, int n, int span_bits, uint32_t* info, void* ws, size_t ws_bytes) {
    if (!c || !files || !info || !ws) return fail(c, -1, "ir_png_decode: null argument");
    if (n < 1) return fail(c, -1, "ir_png_decode: n %d", n);
    if (span_bits < 256 || span_bits > (1 << 20) || span_bits % 32) return fail(c, -1, "ir_png_decode: span_bits %d is no multiple of 32 in 256 .. 2^20", span_bits);
    if (reinterpret_cast<uintptr_t>(info) & 3) return fail(c, -1, "ir_png_decode: misaligned info pointer");
    int mh = 0, mw = 0;
    uint32_t ms = 0;
    for (int i = 0; i < n; ++i) {   // every file is checked before the first launch
        const char* why;
        if (ir_png_decode_check(&files[i], &why)) return fail(c, -1, "ir_png_decode: file %d (%d x %d): %s", i, files[i].h, files[i].w, why);
        mh = std::max(mh, files[i].h), mw = std::max(mw, files[i].w), ms = std::max(ms, files[i].stream_bytes);
    }
    IrPngLayout L;   // one layout for the batch: the sections lie where ir_workspace_bytes's arguments put them
    if (!ir_png_decode_layout(mh, mw, ms, span_bits, &L)) return fail(c, -1, "ir_png_decode: %d x %d with %u stream bytes is outside the contract", mh, mw, ms);
    if (int e = check_ws(c, "ir_png_decode", ws, ws_bytes, L.total, 256)) return e;
    use_ctx(c);
    for (int i = 0; i < n; ++i)
        if (ir_launch_png_decode(&files[i], span_bits, info + i, ws, L, (hipStream_t)stream)) return fail(c, -100, "ir_png_decode: launch failed (file %d)", i);
    return 0;
}

// ---------------------------------------------------------------- Pillow's 8-bit resampling (resample.hip)
// The tables of Resample.c's precompute_coeffs + normalize_coeffs_8bpc. Plain double arithmetic in Pillow's order of operations (no contraction
// into fused multiply-adds): the quantised coefficients have to be Pillow's to the last bit.
#pragma clang fp contract(off)
static double rs_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double rs_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3) : 0.0; }
static double rs_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
static double rs_support(int filter) { return filter == IR_RESAMPLE_LANCZOS ? 3.0 : filter == IR_RESAMPLE_BOX ? 0.5 : 2.0; }
struct RsAxis {
    double scale, filterscale, support;
    int ksize;
};
static RsAxis rs_axis(int in, int out, int filter) {
    RsAxis a;
    a.filterscale = a.scale = (double)(float)in / out;
    if (a.filterscale < 1.0) a.filterscale = 1.0;
    a.support = rs_support(filter) * a.filterscale;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}
static void rs_tables(int in, int out, int filter, int* bounds, int* kk) {
    const RsAxis a = rs_axis(in, out, filter);
    std::vector<double> w(a.ksize);
    const double ss = 1.0 / a.filterscale;
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * a.scale;
        double ww = 0.0;
        int xmin = (int)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + a.support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            w[x] = filter == IR_RESAMPLE_LANCZOS ? rs_lanczos(arg) : filter == IR_RESAMPLE_BOX ? rs_box(arg) : rs_bicubic(arg);
            ww += w[x];
        }
        int* k = kk + (size_t)xx * a.ksize;
        for (int x = 0; x < a.ksize; ++x) {
            double v = x < xmax ? w[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}
#pragma clang fp contract(fast)
static bool rs_args_ok(int in_h, int in_w, int out_h, int out_w, int filter) {
    return in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1 && (filter == IR_RESAMPLE_BICUBIC || filter == IR_RESAMPLE_LANCZOS || filter == IR_RESAMPLE_BOX);
}
// ints of the plan: the header, then per pass that runs 2 bounds + ksize coefficients per output index
static size_t rs_plan_ints(int in_h, int in_w, int out_h, int out_w, int filter, int* hd) {
    size_t at = IR_RESAMPLE_HEADER;
    int h[IR_RESAMPLE_HEADER] = {IR_RESAMPLE_MAGIC, in_h, in_w, out_h, out_w, filter};
    if (in_w != out_w) {
        h[6] = rs_axis(in_w, out_w, filter).ksize;
        h[8] = (int)at; at += 2 * (size_t)out_w;
        h[9] = (int)at; at += (size_t)out_w * h[6];
    }
    if (in_h != out_h) {
        h[7] = rs_axis(in_h, out_h, filter).ksize;
        h[10] = (int)at; at += 2 * (size_t)out_h;
        h[11] = (int)at; at += (size_t)out_h * h[7];
    }
    h[12] = (int)at;
    if (hd) memcpy(hd, h, sizeof h);
    return at;
}
size_t ir_resample_plan_bytes(int in_h, int in_w, int out_h, int out_w, int filter) {
    if (!rs_args_ok(in_h, in_w, out_h, out_w, filter)) return 0;
    const size_t ints = rs_plan_ints(in_h, in_w, out_h, out_w, filter, nullptr);
    return ints > 0x7fffffffu ? 0 : 4 * ints;   // the offsets are ints
}
int ir_resample_plan(int in_h, int in_w, int out_h, int out_w, int filter, void* host_plan, size_t bytes) {
    const size_t need = ir_resample_plan_bytes(in_h, in_w, out_h, out_w, filter);
    if (!host_plan || !need || bytes < need) return -1;
    int* p = static_cast<int*>(host_plan);
    rs_plan_ints(in_h, in_w, out_h, out_w, filter, p);
    if (in_w != out_w) rs_tables(in_w, out_w, filter, p + p[8], p + p[9]);
    if (in_h != out_h) rs_tables(in_h, out_h, filter, p + p[10], p + p[11]);
    return 0;
}
static size_t rs_inter_pitch(int out_w) { return (3 * (size_t)out_w + 3) & ~(size_t)3; }
static size_t rs_workspace(int n, int in_h, int out_w) { return ((size_t)n * in_h * rs_inter_pitch(out_w) + 255) & ~(size_t)255; }
int ir_resample_u8(ir_ctx* c, void* stream, const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int full_h,
                   int full_w, long out_pitch, const void* plan_dev, void* ws, size_t ws_bytes) {
    if (!c || !in || !out || !plan_dev) return fail(c, -1, "ir_resample_u8: null argument");
    if (n < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || full_h < out_h || full_w < out_w || in_pitch < 3L * in_w || out_pitch < 3L * full_w)
        return fail(c, -1, "ir_resample_u8: bad size (n %d, %d x %d pitch %ld -> %d x %d in %d x %d pitch %ld)", n, in_h, in_w, in_pitch, out_h, out_w, full_h,
                    full_w, out_pitch);
    const bool both = in_h != out_h && in_w != out_w;
    if (both && (!ws || ws_bytes < rs_workspace(n, in_h, out_w) || (reinterpret_cast<uintptr_t>(ws) & 3)))
        return fail(c, -1, "ir_resample_u8: workspace missing, too small or unaligned (%zu < %zu)", ws_bytes, rs_workspace(n, in_h, out_w));
    if (reinterpret_cast<uintptr_t>(plan_dev) & 3) return fail(c, -1, "ir_resample_u8: plan not aligned to 4 bytes");
    use_ctx(c);
    if (ir_launch_resample_u8(in, n, in_h, in_w, in_pitch, out, out_h, out_w, full_h, full_w, out_pitch, static_cast<const int*>(plan_dev),
                              static_cast<uint8_t*>(ws), (long)rs_inter_pitch(out_w), (hipStream_t)stream))
        return fail(c, -100, "ir_resample_u8: launch failed (more than 65535 images or rows)");
    return 0;
}
int ir_resample_u8_window(ir_ctx* c, void* stream, const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int y0,
                          int x0, int win_h, int win_w, int full_h, int full_w, long out_pitch, const void* plan_dev, void* ws, size_t ws_bytes) {
    if (!c || !in || !out || !plan_dev) return fail(c, -1, "ir_resample_u8_window: null argument");
    if (n < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || in_pitch < 3L * in_w)
        return fail(c, -1, "ir_resample_u8_window: bad size (n %d, %d x %d pitch %ld -> %d x %d)", n, in_h, in_w, in_pitch, out_h, out_w);
    if (y0 < 0 || x0 < 0 || win_h < 1 || win_w < 1 || y0 > out_h - win_h || x0 > out_w - win_w)
        return fail(c, -1, "ir_resample_u8_window: the window %d x %d at (%d, %d) lies outside the %d x %d result", win_h, win_w, y0, x0, out_h, out_w);
    if (full_h < win_h || full_w < win_w || out_pitch < 3L * full_w)
        return fail(c, -1, "ir_resample_u8_window: bad destination (window %d x %d in %d x %d pitch %ld)", win_h, win_w, full_h, full_w, out_pitch);
    const bool both = in_h != out_h && in_w != out_w;
    if (both && (!ws || ws_bytes < rs_workspace(n, in_h, win_w) || (reinterpret_cast<uintptr_t>(ws) & 3)))
        return fail(c, -1, "ir_resample_u8_window: workspace missing, too small or unaligned (%zu < %zu)", ws_bytes, rs_workspace(n, in_h, win_w));
    if (reinterpret_cast<uintptr_t>(plan_dev) & 3) return fail(c, -1, "ir_resample_u8_window: plan not aligned to 4 bytes");
    use_ctx(c);
    if (ir_launch_resample_u8_window(in, n, in_h, in_w, in_pitch, out, out_h, out_w, y0, x0, win_h, win_w, full_h, full_w, out_pitch,
                                     static_cast<const int*>(plan_dev), static_cast<uint8_t*>(ws), (long)rs_inter_pitch(win_w), (hipStream_t)stream))
        return fail(c, -100, "ir_resample_u8_window: launch failed (more than 65535 images or rows)");
    return 0;
}

// ---------------------------------------------------------------- PSNR-Y / SSIM-Y (metrics.hip)
// two doubles per tile of the 'valid' SSIM map (at least one tile, so that every size from 1 up has a positive answer)
static size_t metrics_workspace(int n, int h, int w) {
    const size_t tx = w > 10 ? ((size_t)w - 10 + IR_METRICS_TW - 1) / IR_METRICS_TW : 1, ty = h > 10 ? ((size_t)h - 10 + IR_METRICS_TH - 1) / IR_METRICS_TH : 1;
    return ((size_t)n * tx * ty * 2 * sizeof(double) + 255) & ~(size_t)255;
}
int ir_metrics_y(ir_ctx* c, void* stream, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w,
                 double* out, void* ws, size_t ws_bytes) {
    if (!c || !a || !b || !out || !ws) return fail(c, -1, "ir_metrics_y: null argument");
    if (int e = check_rect(c, "ir_metrics_y", "the window needs 11 x 11", n, h, w, 11, {{a_rows, a_pitch}, {b_rows, b_pitch}})) return e;
    if (int e = check_ws(c, "ir_metrics_y", ws, ws_bytes, metrics_workspace(n, h, w), 8)) return e;
    if (int e = check_out8(c, "ir_metrics_y", out)) return e;
    if (!c->luma_tab) return fail(c, -1, "ir_metrics_y: the context has no luma tables");
    use_ctx(c);
    if (ir_launch_metrics_y(a, a_rows, a_pitch, b, b_rows, b_pitch, n, h, w, c->luma_tab, static_cast<double*>(ws), out, (hipStream_t)stream))
        return fail(c, -100, "ir_metrics_y: launch failed (more than 65535 images or tile rows)");
    return 0;
}

// ---------------------------------------------------------------- LPIPS (lpips.hip)
int ir_lpips_scale_table(float* tab) {
    if (!tab) return -1;
    static const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
            volatile float x = (float)v / 255.0f;
            volatile float y = 2.0f * x;
            volatile float z = y - 1.0f;
            volatile float u = z - shift[ch];
            tab[256 * ch + v] = u / scale[ch];
        }
    return 0;
}

int ir_lpips_configure(ir_ctx* c) {
    if (!c) return -1;
    static const int shape[5][3] = {{3, 64, 11}, {64, 192, 5}, {192, 384, 3}, {384, 256, 3}, {256, 256, 3}};   // cin, cout, k
    HIPOK(c, hipSetDevice(c->device));
    c->lpips.ok = false;
    ir_ctx::Lpips m;
    const char* const who = "ir_lpips_configure";
    const float* src[5];
    for (int k = 0; k < 5; ++k) {   // every tensor is looked up before anything is replaced
        const int cin = shape[k][0], cout = shape[k][1], ks = shape[k][2];
        if (!(src[k] = exact_f32(c, who, "AlexNet's", fmt("lpips.c%d.w", k + 1), (size_t)cout * cin * ks * ks)) ||
            !(m.b[k] = exact_f32(c, who, "AlexNet's", fmt("lpips.c%d.b", k + 1), (size_t)cout)) ||
            !(m.lin[k] = exact_f32(c, who, "AlexNet's", fmt("lpips.lin%d", k + 1), (size_t)cout)))
            return -2;
    }
    std::vector<void*>& own = c->own[OWN_LPIPS];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[3 * 256];
    ir_lpips_scale_table(tab);
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m.tab)) return e;
    for (int k = 0; k < 5; ++k) {
        const int cout = shape[k][1];
        std::vector<float> t;
        if (int e = repacked_conv(c, src[k], shape[k][0], cout, shape[k][2], t)) return e;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &m.w[k])) return e;
        // copies of the bias and the lin head: the binding does not depend on later uploads under these names
        for (const float** q : {&m.b[k], &m.lin[k]})
            if (int e = own_copy(c, own, *q, (size_t)cout * 4, hipMemcpyDeviceToDevice, q)) return e;
    }
    m.ok = true;
    c->lpips = m;
    ++c->generation;
    return 0;
}

int ir_lpips(ir_ctx* c, void* stream, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w,
             double* out, void* ws, size_t ws_bytes) {
    if (!c || !a || !b || !out || !ws) return fail(c, -1, "ir_lpips: null argument");
    if (int e = check_rect(c, "ir_lpips", "AlexNet's five stages need 31 x 31", n, h, w, 31, {{a_rows, a_pitch}, {b_rows, b_pitch}})) return e;
    IrLpipsPlan pl;
    if (ir_lpips_plan(n, h, w, &pl)) return fail(c, -1, "ir_lpips: n %d of %d x %d is more than one call takes (2^31 output pixels, 65535 pairs)", n, h, w);
    if (int e = check_ws(c, "ir_lpips", ws, ws_bytes, pl.total, 256)) return e;
    if (int e = check_out8(c, "ir_lpips", out)) return e;
    if (!c->lpips.ok) return fail(c, -12, "ir_lpips: LPIPS not configured (ir_lpips_configure)");
    use_ctx(c);
    if (ir_launch_lpips(a, a_rows, a_pitch, b, b_rows, b_pitch, n, h, w, c->lpips.tab, c->lpips.w, c->lpips.b, c->lpips.lin, ws, out, (hipStream_t)stream))
        return fail(c, -100, "ir_lpips: launch failed");
    return 0;
}

// ---------------------------------------------------------------- DISTS (dists.hip)
int ir_dists_scale_table(float* tab) {
    if (!tab) return -1;
    static const float mean[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
            volatile float x = (float)v / 255.0f;
            volatile float u = x - mean[ch];
            tab[256 * ch + v] = u / std3[ch];
        }
    return 0;
}

int ir_dists_configure(ir_ctx* c) {
    if (!c) return -1;
    static const int width[IR_DISTS_CONVS + 1] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};   // conv k: width[k] -> width[k + 1]
    HIPOK(c, hipSetDevice(c->device));
    c->dists.ok = false;
    IrDistsModel m;
    const char* const who = "ir_dists_configure";
    const float* src[IR_DISTS_CONVS];
    for (int k = 0; k < IR_DISTS_CONVS; ++k)   // every tensor is looked up before anything is replaced
        if (!(src[k] = exact_f32(c, who, "VGG-16's", fmt("dists.c%d.w", k + 1), (size_t)width[k + 1] * width[k] * 9)) ||
            !(m.b[k] = exact_f32(c, who, "VGG-16's", fmt("dists.c%d.b", k + 1), (size_t)width[k + 1])))
            return -2;
    if (!(m.alpha = exact_f32(c, who, "DISTS'", "dists.alpha", IR_DISTS_CHANNELS)) || !(m.beta = exact_f32(c, who, "DISTS'", "dists.beta", IR_DISTS_CHANNELS))) return -2;
    std::vector<void*>& own = c->own[OWN_DISTS];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[3 * 256], x01[256];
    ir_dists_scale_table(tab);
    for (int v = 0; v < 256; ++v) x01[v] = (float)v / 255.0f;
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m.tab)) return e;
    if (int e = own_copy(c, own, x01, sizeof x01, hipMemcpyHostToDevice, &m.x01)) return e;
    for (int k = 0; k < IR_DISTS_CONVS; ++k) {
        std::vector<float> t;
        if (int e = repacked_conv(c, src[k], width[k], width[k + 1], 3, t)) return e;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &m.w[k])) return e;
        if (int e = own_copy(c, own, m.b[k], (size_t)width[k + 1] * 4, hipMemcpyDeviceToDevice, &m.b[k])) return e;   // a copy: later uploads do not reach the binding
    }
    std::vector<float> ab(2 * IR_DISTS_CHANNELS);
    HIPOK(c, hipMemcpy(ab.data(), m.alpha, IR_DISTS_CHANNELS * 4, hipMemcpyDeviceToHost));
    HIPOK(c, hipMemcpy(ab.data() + IR_DISTS_CHANNELS, m.beta, IR_DISTS_CHANNELS * 4, hipMemcpyDeviceToHost));
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < IR_DISTS_CHANNELS; ++i) {
        sa += (double)ab[i];
        sb += (double)ab[IR_DISTS_CHANNELS + i];
    }
    m.wsum = sa + sb;
    if (int e = own_copy(c, own, ab.data(), IR_DISTS_CHANNELS * 4, hipMemcpyHostToDevice, &m.alpha)) return e;
    if (int e = own_copy(c, own, ab.data() + IR_DISTS_CHANNELS, IR_DISTS_CHANNELS * 4, hipMemcpyHostToDevice, &m.beta)) return e;
    m.ok = true;
    c->dists = m;
    ++c->generation;
    return 0;
}

int ir_dists(ir_ctx* c, void* stream, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w,
             double* out, double* moments, void* ws, size_t ws_bytes) {
    if (!c || !a || !b || !out || !ws) return fail(c, -1, "ir_dists: null argument");
    if (int e = check_rect(c, "ir_dists", "this library scores DISTS from 16 x 16", n, h, w, IR_DISTS_MIN_EDGE, {{a_rows, a_pitch}, {b_rows, b_pitch}})) return e;
    IrDistsPlan pl;
    if (ir_dists_plan(n, h, w, &pl)) return fail(c, -1, "ir_dists: n %d of %d x %d is more than one call takes (2^31 pixels, 65535 pairs)", n, h, w);
    if (int e = check_ws(c, "ir_dists", ws, ws_bytes, pl.total, 256)) return e;
    if (int e = check_out8(c, "ir_dists", out)) return e;
    if (int e = check_out8(c, "ir_dists", moments)) return e;
    if (!c->dists.ok) return fail(c, -14, "ir_dists: DISTS not configured (ir_dists_configure)");
    use_ctx(c);
    if (ir_launch_dists(c->dists, a, a_rows, a_pitch, b, b_rows, b_pitch, n, h, w, ws, out, moments, (hipStream_t)stream)) return fail(c, -100, "ir_dists: launch failed");
    return 0;
}

// ---------------------------------------------------------------- FID's Inception-v3 features (fid.hip)
// The tables of the two resizes to 299 x 299. clean: Resample.c's precompute_coeffs for BICUBIC as doubles (Pillow's mode-F path keeps them as they
// are), in Pillow's order of operations. legacy: torch's bilinear indices and weights in fp32, src = fmaf(scale, i + 0.5, -0.5) as its CPU kernels
// compute it where the processor fuses; the two weights are stored as doubles (exactly).
extern "C++" int ir_fid_tables_layout(int h, int w, int mode, IrFidTables* t) {
    if (h < 1 || w < 1 || (mode != IR_FID_RESIZE_CLEAN && mode != IR_FID_RESIZE_LEGACY)) return -1;
    t->kx = mode == IR_FID_RESIZE_CLEAN ? rs_axis(w, IR_FID_SIZE, IR_RESAMPLE_BICUBIC).ksize : 2;
    t->ky = mode == IR_FID_RESIZE_CLEAN ? rs_axis(h, IR_FID_SIZE, IR_RESAMPLE_BICUBIC).ksize : 2;
    t->xb = 0;
    t->yb = 2 * IR_FID_SIZE * sizeof(int);
    t->xk = 4 * IR_FID_SIZE * sizeof(int) + 8;   // 4792 + 8: a multiple of 8
    t->yk = t->xk + (size_t)IR_FID_SIZE * t->kx * sizeof(double);
    t->total = t->yk + (size_t)IR_FID_SIZE * t->ky * sizeof(double);
    return 0;
}
#pragma clang fp contract(off)
static void fid_clean_axis(int in, int ksize, int* bounds, double* kk) {
    const RsAxis a = rs_axis(in, IR_FID_SIZE, IR_RESAMPLE_BICUBIC);
    const double ss = 1.0 / a.filterscale;
    for (int xx = 0; xx < IR_FID_SIZE; ++xx) {
        const double center = (xx + 0.5) * a.scale;
        double ww = 0.0;
        int xmin = (int)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + a.support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) k[x] = 0.0;
        for (int x = 0; x < xmax; ++x) {
            k[x] = rs_bicubic((x + xmin - center + 0.5) * ss);
            ww += k[x];
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}
static void fid_legacy_axis(int in, int* idx, double* lam) {
    const float scale = (float)in / (float)IR_FID_SIZE;
    for (int i = 0; i < IR_FID_SIZE; ++i) {
        float real = fmaf(scale, (float)i + 0.5f, -0.5f);
        if (real < 0.f) real = 0.f;
        const int i0 = std::min((int)floorf(real), in - 1);
        const float l1 = std::min(std::max(real - (float)i0, 0.f), 1.f);
        idx[2 * i] = i0;
        idx[2 * i + 1] = std::min(i0 + 1, in - 1);
        lam[2 * i] = (double)(1.f - l1);
        lam[2 * i + 1] = (double)l1;
    }
}
#pragma clang fp contract(fast)
size_t ir_fid_resize_plan_bytes(int h, int w, int mode) {
    IrFidTables t;
    return ir_fid_tables_layout(h, w, mode, &t) ? 0 : t.total;
}
int ir_fid_resize_plan(int h, int w, int mode, void* host_tables, size_t bytes) {
    IrFidTables t;
    if (!host_tables || ir_fid_tables_layout(h, w, mode, &t) || bytes < t.total || (reinterpret_cast<uintptr_t>(host_tables) & 7)) return -1;
    char* b = static_cast<char*>(host_tables);
    memset(b, 0, t.total);
    int *xb = reinterpret_cast<int*>(b + t.xb), *yb = reinterpret_cast<int*>(b + t.yb);
    double *xk = reinterpret_cast<double*>(b + t.xk), *yk = reinterpret_cast<double*>(b + t.yk);
    if (mode == IR_FID_RESIZE_CLEAN) {
        fid_clean_axis(w, t.kx, xb, xk);
        fid_clean_axis(h, t.ky, yb, yk);
    } else {
        fid_legacy_axis(w, xb, xk);
        fid_legacy_axis(h, yb, yk);
    }
    return 0;
}

int ir_fid_configure(ir_ctx* c) {
    if (!c) return -1;
    HIPOK(c, hipSetDevice(c->device));
    c->fid.ok = false;
    IrFidModel m;
    const char* const who = "ir_fid_configure";
    const IrFidConv* convs = ir_fid_convs();
    static const char* const parts[4] = {"bn_w", "bn_b", "bn_mean", "bn_var"};
    std::vector<const float*> src(IR_FID_CONVS * 5);
    for (int k = 0; k < IR_FID_CONVS; ++k) {   // every tensor is looked up before anything is replaced
        const IrFidConv& v = convs[k];
        if (!(src[5 * k] = exact_f32(c, who, "Inception-v3's", fmt("fid.%s.w", v.name), (size_t)v.cout * v.cin * v.kh * v.kw))) return -2;
        for (int j = 0; j < 4; ++j)
            if (!(src[5 * k + 1 + j] = exact_f32(c, who, "Inception-v3's", fmt("fid.%s.%s", v.name, parts[j]), (size_t)v.cout))) return -2;
    }
    std::vector<void*>& own = c->own[OWN_FID];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float x01[256];
    for (int v = 0; v < 256; ++v) x01[v] = (float)v / 255.0f;
    if (int e = own_copy(c, own, x01, sizeof x01, hipMemcpyHostToDevice, &m.x01)) return e;
    for (int k = 0; k < IR_FID_CONVS; ++k) {
        const IrFidConv& v = convs[k];
        const int cin = v.cin == 3 ? 4 : v.cin, K = v.kh * v.kw * cin, npad = (v.cout + 63) / 64 * 64;
        std::vector<float> w((size_t)v.cout * v.cin * v.kh * v.kw), t((size_t)pad32(K) * npad, 0.f), bn[4];
        HIPOK(c, hipMemcpy(w.data(), src[5 * k], w.size() * 4, hipMemcpyDeviceToHost));
        for (int j = 0; j < 4; ++j) {
            bn[j].resize(v.cout);
            HIPOK(c, hipMemcpy(bn[j].data(), src[5 * k + 1 + j], (size_t)v.cout * 4, hipMemcpyDeviceToHost));
        }
        for (int o = 0; o < v.cout; ++o)
            for (int ci = 0; ci < v.cin; ++ci)
                for (int ky = 0; ky < v.kh; ++ky)
                    for (int kx = 0; kx < v.kw; ++kx)
                        t[(size_t)((ky * v.kw + kx) * cin + ci) * npad + o] = w[(((size_t)o * v.cin + ci) * v.kh + ky) * v.kw + kx];
        std::vector<float> scale(v.cout), shift(v.cout);
        for (int o = 0; o < v.cout; ++o) {   // eval-mode BatchNorm, eps 1e-3: y = (x - mean) / sqrt(var + eps) * w + b, folded in fp64
            const double sc = (double)bn[0][o] / sqrt((double)bn[3][o] + 1e-3);
            scale[o] = (float)sc;
            shift[o] = (float)((double)bn[1][o] - (double)bn[2][o] * sc);
        }
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &m.w[k])) return e;
        if (int e = own_copy(c, own, scale.data(), scale.size() * 4, hipMemcpyHostToDevice, &m.scale[k])) return e;
        if (int e = own_copy(c, own, shift.data(), shift.size() * 4, hipMemcpyHostToDevice, &m.shift[k])) return e;
    }
    m.ok = true;
    c->fid = m;
    ++c->generation;
    return 0;
}

int ir_fid_features(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, int mode, const void* tables, double* features,
                    double* block_means, float* resized, void* ws, size_t ws_bytes) {
    if (!c || !img || !tables || !features || !ws) return fail(c, -1, "ir_fid_features: null argument");
    if (int e = check_rect(c, "ir_fid_features", "this library takes FID's features from 2 x 2", n, h, w, IR_FID_MIN_EDGE, {{rows, pitch}},
                           mode != IR_FID_RESIZE_CLEAN && mode != IR_FID_RESIZE_LEGACY))
        return e;
    IrFidPlan pl;
    if (ir_fid_plan(n, &pl)) return fail(c, -1, "ir_fid_features: n %d is more than one call takes (%d)", n, IR_FID_MAX_N);
    if (int e = check_ws(c, "ir_fid_features", ws, ws_bytes, pl.total, 256)) return e;
    if (int e = check_out8(c, "ir_fid_features", features)) return e;
    if (int e = check_out8(c, "ir_fid_features", block_means)) return e;
    if (int e = check_out8(c, "ir_fid_features", tables)) return e;
    if (reinterpret_cast<uintptr_t>(resized) & 3) return fail(c, -1, "ir_fid_features: resized not aligned to 4 bytes");
    if (!c->fid.ok) return fail(c, -14, "ir_fid_features: FID not configured (ir_fid_configure)");
    use_ctx(c);
    if (ir_launch_fid(c->fid, img, rows, pitch, n, h, w, mode, tables, features, block_means, resized, ws, (hipStream_t)stream))
        return fail(c, -100, "ir_fid_features: launch failed");
    return 0;
}

// ---------------------------------------------------------------- CLIP-IQA (clipiqa.hip)
int ir_clipiqa_scale_table(float* tab) {
    if (!tab) return -1;
    static const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, std3[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int ch = 0; ch < 3; ++ch)
        for (int v = 0; v < 256; ++v) {   // every step rounded to fp32, in the model's order
            volatile float x = (float)v / 255.0f;
            volatile float y = x - mean[ch];
            tab[256 * ch + v] = y / std3[ch];
        }
    return 0;
}

namespace {
struct ClipConvSrc { std::string conv, bn; int cin, cout, ks; IrClipConv* dst; };
}  // namespace

int ir_clipiqa_configure(ir_ctx* c, const int* layers, int width, int heads, int out_dim, int n_pairs, float logit_scale_exp) {
    if (!c || !layers) return fail(c, -1, "ir_clipiqa_configure: null argument");
    int n_blocks = 0;
    for (int l = 0; l < 4; ++l) {
        if (layers[l] < 1) return fail(c, -1, "ir_clipiqa_configure: layer %d has %d blocks", l + 1, layers[l]);
        n_blocks += layers[l];
    }
    if (n_blocks > IR_CLIPIQA_MAX_BLOCKS) return fail(c, -1, "ir_clipiqa_configure: %d blocks, at most %d", n_blocks, IR_CLIPIQA_MAX_BLOCKS);
    if (width < 64 || width % 64 || heads < 1 || (width * 32) % heads || out_dim < 1 || n_pairs < 1 || n_pairs > 64 || !(logit_scale_exp > 0.f))
        return fail(c, -1, "ir_clipiqa_configure: unsupported model (width %d must be a multiple of 64, heads %d must divide %d, out_dim %d, %d pairs)", width,
                    heads, width * 32, out_dim, n_pairs);
    HIPOK(c, hipSetDevice(c->device));
    c->clipiqa.ok = false;
    auto m = std::make_unique<IrClipiqaModel>();
    for (int l = 0; l < 4; ++l) m->layers[l] = layers[l];
    m->width = width; m->heads = heads; m->out_dim = out_dim; m->n_pairs = n_pairs; m->n_blocks = n_blocks; m->logit_scale = (double)logit_scale_exp;
    std::vector<ClipConvSrc> convs;
    convs.push_back({"clipiqa.conv1", "clipiqa.bn1", 3, width / 2, 3, &m->stem[0]});
    convs.push_back({"clipiqa.conv2", "clipiqa.bn2", width / 2, width / 2, 3, &m->stem[1]});
    convs.push_back({"clipiqa.conv3", "clipiqa.bn3", width / 2, width, 3, &m->stem[2]});
    int inplanes = width, bi = 0;
    for (int l = 0; l < 4; ++l) {
        const int planes = width << l;
        for (int i = 0; i < layers[l]; ++i, ++bi) {
            IrClipBlock& b = m->blocks[bi];
            b.stride = (i == 0 && l > 0) ? 2 : 1;
            b.has_down = b.stride == 2 || inplanes != planes * 4;
            const std::string base = fmt("clipiqa.layer%d.%d.", l + 1, i);
            convs.push_back({base + "conv1", base + "bn1", inplanes, planes, 1, &b.c1});
            convs.push_back({base + "conv2", base + "bn2", planes, planes, 3, &b.c2});
            convs.push_back({base + "conv3", base + "bn3", planes, planes * 4, 1, &b.c3});
            if (b.has_down) convs.push_back({base + "downsample.0", base + "downsample.1", inplanes, planes * 4, 1, &b.down});
            inplanes = planes * 4;
        }
    }
    const int C = width * 32;
    auto tensor = [&](const std::string& name, size_t floats) { return exact_f32(c, "ir_clipiqa_configure", "the configured model's", name, floats); };
    // every tensor is looked up before anything is replaced
    struct Lin { const char* name; int rows, cols; const float **w, **b; };
    const Lin lins[4] = {{"q_proj", C, C, &m->qw, &m->qb}, {"k_proj", C, C, &m->kw, &m->kb}, {"v_proj", C, C, &m->vw, &m->vb}, {"c_proj", out_dim, C, &m->cw, &m->cb}};
    for (const ClipConvSrc& s : convs) {
        if (!tensor(s.conv + ".weight", (size_t)s.cout * s.cin * s.ks * s.ks)) return -2;
        for (const char* v : {".weight", ".bias", ".running_mean", ".running_var"})
            if (!tensor(s.bn + v, (size_t)s.cout)) return -2;
    }
    for (const Lin& l : lins)
        if (!tensor(fmt("clipiqa.attnpool.%s.weight", l.name), (size_t)l.rows * l.cols) || !tensor(fmt("clipiqa.attnpool.%s.bias", l.name), (size_t)l.rows))
            return -2;
    if (!tensor("clipiqa.text", (size_t)2 * n_pairs * out_dim)) return -2;

    std::vector<void*>& own = c->own[OWN_CLIPIQA];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[3 * 256];
    ir_clipiqa_scale_table(tab);
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m->tab)) return e;
    for (const ClipConvSrc& s : convs) {   // the repacked weights, and BatchNorm folded in fp64
        std::vector<float> t, bn[4], sc(s.cout), sh(s.cout);
        if (int e = repacked_conv(c, tensor(s.conv + ".weight", (size_t)s.cout * s.cin * s.ks * s.ks), s.cin, s.cout, s.ks, t)) return e;
        int k = 0;
        for (const char* v : {".weight", ".bias", ".running_mean", ".running_var"}) {
            bn[k].resize(s.cout);
            HIPOK(c, hipMemcpy(bn[k].data(), tensor(s.bn + v, (size_t)s.cout), (size_t)s.cout * 4, hipMemcpyDeviceToHost));
            ++k;
        }
        for (int o = 0; o < s.cout; ++o) {   // scale = g / sqrt(var + eps), shift = b - mean scale, each rounded to fp32 once
            const double scale = (double)bn[0][o] / sqrt((double)bn[3][o] + 1e-5);
            sc[o] = (float)scale;
            sh[o] = (float)((double)bn[1][o] - (double)bn[2][o] * scale);
        }
        s.dst->cin = s.cin; s.dst->cout = s.cout; s.dst->ks = s.ks;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &s.dst->w)) return e;
        if (int e = own_copy(c, own, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, &s.dst->scale)) return e;
        if (int e = own_copy(c, own, sh.data(), sh.size() * 4, hipMemcpyHostToDevice, &s.dst->shift)) return e;
    }
    // copies of the linears and the text rows: the binding does not depend on later uploads under these names
    for (const Lin& l : lins) {
        const size_t nw = (size_t)l.rows * l.cols, nb = (size_t)l.rows;
        if (int e = own_copy(c, own, tensor(fmt("clipiqa.attnpool.%s.weight", l.name), nw), nw * 4, hipMemcpyDeviceToDevice, l.w)) return e;
        if (int e = own_copy(c, own, tensor(fmt("clipiqa.attnpool.%s.bias", l.name), nb), nb * 4, hipMemcpyDeviceToDevice, l.b)) return e;
    }
    const size_t nt = (size_t)2 * n_pairs * out_dim;
    if (int e = own_copy(c, own, tensor("clipiqa.text", nt), nt * 4, hipMemcpyDeviceToDevice, &m->text)) return e;
    m->ok = true;
    c->clipiqa = *m;
    ++c->generation;
    return 0;
}

int ir_clipiqa(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws, size_t ws_bytes) {
    if (!c || !img || !scores || !ws) return fail(c, -1, "ir_clipiqa: null argument");
    if (int e = check_rect(c, "ir_clipiqa", "the tower's last map needs 32 x 32", n, h, w, 32, {{rows, pitch}})) return e;
    if (!c->clipiqa.ok) return fail(c, -13, "ir_clipiqa: CLIP-IQA not configured (ir_clipiqa_configure)");
    IrClipiqaPlan pl;
    if (ir_clipiqa_plan(c->clipiqa, n, h, w, &pl)) return fail(c, -1, "ir_clipiqa: n %d of %d x %d is more than one call takes (2^31 output pixels, 65535 images)", n, h, w);
    if (int e = check_ws(c, "ir_clipiqa", ws, ws_bytes, pl.total, 256)) return e;
    if ((reinterpret_cast<uintptr_t>(scores) & 7) || (reinterpret_cast<uintptr_t>(feat) & 3)) return fail(c, -1, "ir_clipiqa: scores / feat not aligned");
    use_ctx(c);
    if (ir_launch_clipiqa(c->clipiqa, img, rows, pitch, n, h, w, scores, feat, ws, (hipStream_t)stream)) return fail(c, -100, "ir_clipiqa: launch failed");
    return 0;
}

// ---------------------------------------------------------------- MUSIQ (musiq.hip)
int ir_musiq_input_table(float* tab) {
    if (!tab) return -1;
    ir_musiq_input_table_host(tab);
    return 0;
}

int ir_musiq_layout(int h, int w, int patch, int grid, int n_scales, const int* longer, int* out_per_scale, int* spatial_index, int cap) {
    IrMusiqLayout lay;
    if (ir_musiq_layout_host(h, w, patch, grid, n_scales, longer, &lay)) return -1;
    if (spatial_index && cap < lay.patches) return -1;
    for (int k = 0; k < lay.n_scales; ++k) {
        const IrMusiqScale& g = lay.s[k];
        if (out_per_scale) {
            const int v[6] = {g.rh, g.rw, g.count_h, g.count_w, g.pad_top, g.pad_left};
            memcpy(out_per_scale + 6 * k, v, sizeof v);
        }
        if (spatial_index)
            for (int i = 0; i < g.count_h; ++i)
                for (int j = 0; j < g.count_w; ++j) {   // the kernel's expression: torch's nearest interpolation of arange(grid)
                    volatile float fi = (float)i * g.fh, fj = (float)j * g.fw;
                    spatial_index[g.first + i * g.count_w + j] = std::min((int)floorf(fi), grid - 1) * grid + std::min((int)floorf(fj), grid - 1);
                }
    }
    return lay.T;
}

namespace {
// the device tensor [rows][cols] as the host array [cols][ld] at column col0 (a linear's weight as the GEMM's B operand)
int transposed_into(ir_ctx* c, const float* dev_w, int rows, int cols, std::vector<float>& t, int ld, int col0) {
    std::vector<float> w((size_t)rows * cols);
    HIPOK(c, hipMemcpy(w.data(), dev_w, w.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) t[(size_t)k * ld + col0 + r] = w[(size_t)r * cols + k];
    return 0;
}
}  // namespace

int ir_musiq_configure(ir_ctx* c, int patch, int hidden, int mlp, int heads, int layers, int grid, int n_scales, const int* longer) {
    if (!c || !longer) return fail(c, -1, "ir_musiq_configure: null argument");
    if (patch != 32 || heads < 1 || hidden != 64 * heads || mlp < 32 || mlp % 32 || layers < 1 || layers > IR_MUSIQ_MAX_LAYERS || grid < 1 || grid > 1024 ||
        n_scales < 1 || n_scales > IR_MUSIQ_MAX_SCALES)
        return fail(c, -1, "ir_musiq_configure: unsupported model (patch %d must be 32, hidden %d must be 64 x heads %d, mlp %d a multiple of 32, layers %d within 1 .. %d, "
                    "grid %d, %d scales within 1 .. %d)", patch, hidden, heads, mlp, layers, IR_MUSIQ_MAX_LAYERS, grid, n_scales, IR_MUSIQ_MAX_SCALES);
    for (int k = 0; k < n_scales; ++k)
        if (longer[k] < 0) return fail(c, -1, "ir_musiq_configure: scale %d has the longer side %d", k, longer[k]);
    HIPOK(c, hipSetDevice(c->device));
    c->musiq.ok = false;
    auto m = std::make_unique<IrMusiqModel>();
    m->patch = patch; m->hidden = hidden; m->mlp = mlp; m->heads = heads; m->layers = layers; m->grid = grid; m->n_scales = n_scales;
    for (int k = 0; k < n_scales; ++k) m->longer[k] = longer[k];
    const size_t C = hidden, F = mlp, EK = (size_t)8 * 8 * 256;
    struct Conv { const char* name; int cin, cout, ks; const float** dst; };
    const Conv convs[5] = {{"stem.conv", 3, 64, 7, &m->stem_w}, {"block.conv1", 64, 64, 1, &m->cw[0]}, {"block.conv2", 64, 64, 3, &m->cw[1]},
                           {"block.conv3", 64, 256, 1, &m->cw[2]}, {"block.proj", 64, 256, 1, &m->cw[3]}};
    struct Vec { std::string name; size_t floats; const float** dst; };   // tensors that are copied as they are
    std::vector<Vec> vecs;
    auto norm = [&](const std::string& base, size_t nfl, const float** g, const float** b) {
        vecs.push_back({base + ".weight", nfl, g});
        vecs.push_back({base + ".bias", nfl, b});
    };
    norm("musiq.stem.gn", 64, &m->stem_g, &m->stem_b);
    norm("musiq.block.gn1", 64, &m->cg[0], &m->cb[0]);
    norm("musiq.block.gn2", 64, &m->cg[1], &m->cb[1]);
    norm("musiq.block.gn3", 256, &m->cg[2], &m->cb[2]);
    norm("musiq.block.gn_proj", 256, &m->cg[3], &m->cb[3]);
    vecs.push_back({"musiq.embedding.bias", C, &m->emb_b});
    vecs.push_back({"musiq.position_emb", (size_t)grid * grid * C, &m->pos});
    vecs.push_back({"musiq.scale_emb", (size_t)n_scales * C, &m->semb});
    vecs.push_back({"musiq.cls_token", C, &m->cls});
    norm("musiq.final_ln", C, &m->fin_g, &m->fin_b);
    vecs.push_back({"musiq.head.weight", C, &m->head_w});
    vecs.push_back({"musiq.head.bias", 1, &m->head_b});
    for (int l = 0; l < layers; ++l) {
        IrMusiqBlock& b = m->blk[l];
        const std::string base = fmt("musiq.layers.%d.", l);
        norm(base + "ln1", C, &b.ln1g, &b.ln1b);
        norm(base + "ln2", C, &b.ln2g, &b.ln2b);
        vecs.push_back({base + "attn.out.bias", C, &b.ob});
        vecs.push_back({base + "mlp.fc1.bias", F, &b.f1b});
        vecs.push_back({base + "mlp.fc2.bias", C, &b.f2b});
    }
    auto tensor = [&](const std::string& name, size_t floats) { return exact_f32(c, "ir_musiq_configure", "the configured model's", name, floats); };
    // every tensor is looked up before anything is replaced
    for (const Conv& s : convs)
        if (!tensor(fmt("musiq.%s.weight", s.name), (size_t)s.cout * s.cin * s.ks * s.ks)) return -2;
    if (!tensor("musiq.embedding.weight", C * EK)) return -2;
    for (const Vec& v : vecs)
        if (!tensor(v.name, v.floats)) return -2;
    static const char* const qkv[3] = {"q", "k", "v"};
    for (int l = 0; l < layers; ++l) {
        const std::string base = fmt("musiq.layers.%d.", l);
        for (const char* a : {"q", "k", "v", "out"})
            if (!tensor(base + "attn." + a + ".weight", C * C)) return -2;
        for (const char* a : qkv)
            if (!tensor(base + "attn." + a + ".bias", C)) return -2;
        if (!tensor(base + "mlp.fc1.weight", F * C) || !tensor(base + "mlp.fc2.weight", C * F)) return -2;
    }

    std::vector<void*>& own = c->own[OWN_MUSIQ];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[256];
    ir_musiq_input_table_host(tab);
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m->tab)) return e;
    std::vector<float> t;
    for (const Conv& s : convs) {
        if (int e = repacked_conv(c, tensor(fmt("musiq.%s.weight", s.name), (size_t)s.cout * s.cin * s.ks * s.ks), s.cin, s.cout, s.ks, t)) return e;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, s.dst)) return e;
    }
    auto linear = [&](const std::string& name, int rows, int cols, const float** dst) {   // [rows][cols] -> [cols][rows]
        t.assign((size_t)rows * cols, 0.f);
        if (int e = transposed_into(c, tensor(name, (size_t)rows * cols), rows, cols, t, rows, 0)) return e;
        return own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, dst);
    };
    if (int e = linear("musiq.embedding.weight", hidden, (int)EK, &m->emb_w)) return e;
    for (const Vec& v : vecs)
        if (int e = own_copy(c, own, tensor(v.name, v.floats), v.floats * 4, hipMemcpyDeviceToDevice, v.dst)) return e;
    for (int l = 0; l < layers; ++l) {
        IrMusiqBlock& b = m->blk[l];
        const std::string base = fmt("musiq.layers.%d.", l);
        t.assign(C * 3 * C, 0.f);   // q | k | v side by side: one GEMM, the same chain per output
        std::vector<float> bias(3 * C);
        for (int k = 0; k < 3; ++k) {
            if (int e = transposed_into(c, tensor(base + "attn." + qkv[k] + ".weight", C * C), hidden, hidden, t, 3 * hidden, k * hidden)) return e;
            HIPOK(c, hipMemcpy(bias.data() + k * C, tensor(base + "attn." + qkv[k] + ".bias", C), C * 4, hipMemcpyDeviceToHost));
        }
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &b.qkvw)) return e;
        if (int e = own_copy(c, own, bias.data(), bias.size() * 4, hipMemcpyHostToDevice, &b.qkvb)) return e;
        if (int e = linear(base + "attn.out.weight", hidden, hidden, &b.ow)) return e;
        if (int e = linear(base + "mlp.fc1.weight", mlp, hidden, &b.f1w)) return e;
        if (int e = linear(base + "mlp.fc2.weight", hidden, mlp, &b.f2w)) return e;
    }
    m->ok = true;
    c->musiq = *m;
    ++c->generation;
    return 0;
}

int ir_musiq(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws, size_t ws_bytes) {
    if (!c || !img || !scores || !ws) return fail(c, -1, "ir_musiq: null argument");
    if (int e = check_rect(c, "ir_musiq", nullptr, n, h, w, 1, {{rows, pitch}})) return e;
    if (!c->musiq.ok) return fail(c, -13, "ir_musiq: MUSIQ not configured (ir_musiq_configure)");
    IrMusiqLayout lay;
    if (ir_musiq_layout_host(h, w, c->musiq.patch, c->musiq.grid, c->musiq.n_scales, c->musiq.longer, &lay))
        return fail(c, -1, "ir_musiq: a resized side of a %d x %d image rounds to 0", h, w);
    IrMusiqPlan pl;
    if (ir_musiq_plan(c->musiq, n, h, w, &pl)) return fail(c, -1, "ir_musiq: n %d of %d x %d is more than one call takes (4096 images, 2^31 rows)", n, h, w);
    if (int e = check_ws(c, "ir_musiq", ws, ws_bytes, pl.total, 256)) return e;
    if ((reinterpret_cast<uintptr_t>(scores) & 7) || (reinterpret_cast<uintptr_t>(feat) & 3)) return fail(c, -1, "ir_musiq: scores / feat not aligned");
    use_ctx(c);
    if (ir_launch_musiq(c->musiq, img, rows, pitch, n, h, w, scores, feat, ws, (hipStream_t)stream)) return fail(c, -100, "ir_musiq: launch failed");
    return 0;
}

// ---------------------------------------------------------------- MANIQA (maniqa.hip)
int ir_maniqa_input_table(float* tab) {
    if (!tab) return -1;
    ir_maniqa_input_table_host(tab);
    return 0;
}

int ir_maniqa_crops(int h, int w, int crop, int crops, int* out_yx) { return ir_maniqa_crops_host(h, w, crop, crops, out_yx); }

int ir_maniqa_configure(ir_ctx* c, int crop, int patch, int embed, int vit_heads, int vit_mlp, int vit_layers, const int* taps, int window, int swin_heads,
                        int swin_depth, int dim_mlp, float scale) {
    if (!c || !taps) return fail(c, -1, "ir_maniqa_configure: null argument");
    bool bad = patch < 1 || patch > 64 || window < 2 || window > 5 || crop < 1 || crop > 4096 || crop % (patch * window) || embed < 64 || embed % 64 || embed > 4096 ||
               vit_heads < 1 || embed % vit_heads || (embed / vit_heads) % 32 || vit_mlp < 32 || vit_mlp % 32 || vit_layers < 1 || vit_layers > IR_MANIQA_MAX_LAYERS ||
               swin_heads < 1 || swin_heads > 4 || (embed / 2) % swin_heads || (embed / 2 / swin_heads) % 2 || swin_depth < 1 || swin_depth > IR_MANIQA_MAX_DEPTH ||
               dim_mlp < 64 || dim_mlp % 64 || !(scale == scale);
    for (int k = 0; k < 4 && !bad; ++k) bad = taps[k] < 0 || taps[k] >= vit_layers || (k && taps[k] <= taps[k - 1]);
    if (bad)
        return fail(c, -1, "ir_maniqa_configure: unsupported model (crop %d must be a multiple of patch %d x window %d (2 .. 5), embed %d of 64 with %d heads of a multiple of 32, "
                    "vit_mlp %d of 32, layers %d within 1 .. %d, taps ascending below them, 1 .. 4 swin heads (%d) dividing embed / 2, depth %d within 1 .. %d, dim_mlp %d of 64)",
                    crop, patch, window, embed, vit_heads, vit_mlp, vit_layers, IR_MANIQA_MAX_LAYERS, swin_heads, swin_depth, IR_MANIQA_MAX_DEPTH, dim_mlp);
    HIPOK(c, hipSetDevice(c->device));
    c->maniqa.ok = false;
    auto m = std::make_unique<IrManiqaModel>();
    m->crop = crop; m->patch = patch; m->embed = embed; m->vit_heads = vit_heads; m->vit_mlp = vit_mlp; m->vit_layers = vit_layers; m->window = window;
    m->swin_heads = swin_heads; m->swin_depth = swin_depth; m->dim_mlp = dim_mlp; m->scale = scale;
    for (int k = 0; k < 4; ++k) m->taps[k] = taps[k];
    const int G = crop / patch, N = G * G, E = embed, Eh = embed / 2, PK = 3 * patch * patch, RP = (2 * window - 1) * (2 * window - 1);
    struct Vec { std::string name; size_t floats; const float** dst; };   // tensors that are copied as they are
    struct Lin { std::string name; int rows, cols; const float** dst; };  // [rows][cols] -> [cols][rows]
    std::vector<Vec> vecs;
    std::vector<Lin> lins;
    auto block = [&](const std::string& b, int D, int mlp, IrManiqaBlock& k, bool rpb) {
        vecs.push_back({b + "ln1.weight", (size_t)D, &k.ln1g});
        vecs.push_back({b + "ln1.bias", (size_t)D, &k.ln1b});
        vecs.push_back({b + "ln2.weight", (size_t)D, &k.ln2g});
        vecs.push_back({b + "ln2.bias", (size_t)D, &k.ln2b});
        vecs.push_back({b + "attn.qkv.bias", (size_t)3 * D, &k.qkvb});
        vecs.push_back({b + "attn.proj.bias", (size_t)D, &k.pb});
        vecs.push_back({b + "mlp.fc1.bias", (size_t)mlp, &k.f1b});
        vecs.push_back({b + "mlp.fc2.bias", (size_t)D, &k.f2b});
        if (rpb) vecs.push_back({b + "attn.rpb", (size_t)RP * swin_heads, &k.rpb});
        lins.push_back({b + "attn.qkv.weight", 3 * D, D, &k.qkvw});
        lins.push_back({b + "attn.proj.weight", D, D, &k.pw});
        lins.push_back({b + "mlp.fc1.weight", mlp, D, &k.f1w});
        lins.push_back({b + "mlp.fc2.weight", D, mlp, &k.f2w});
    };
    vecs.push_back({"maniqa.vit.patch.bias", (size_t)E, &m->patch_b});
    vecs.push_back({"maniqa.vit.cls_token", (size_t)E, &m->cls});
    vecs.push_back({"maniqa.vit.pos_embed", (size_t)(N + 1) * E, &m->pos});
    lins.push_back({"maniqa.vit.patch.weight", E, PK, &m->patch_w});
    for (int l = 0; l < vit_layers; ++l) block(fmt("maniqa.vit.blocks.%d.", l), E, vit_mlp, m->vit[l], false);
    for (int s = 0; s < 2; ++s) {
        const int cin = s == 0 ? 4 * E : E, D = s == 0 ? E : Eh;
        vecs.push_back({fmt("maniqa.conv%d.bias", s + 1), (size_t)D, &m->convb[s]});
        lins.push_back({fmt("maniqa.conv%d.weight", s + 1), D, cin, &m->convw[s]});
        for (int l = 0; l < IR_MANIQA_SWIN_LAYERS; ++l)
            for (int k = 0; k < swin_depth; ++k) block(fmt("maniqa.swin%d.%d.%d.", s + 1, l, k), D, s == 0 ? dim_mlp : dim_mlp / 2, m->swin[s][l][k], true);
    }
    auto tensor = [&](const std::string& name, size_t floats) { return exact_f32(c, "ir_maniqa_configure", "the configured model's", name, floats); };
    static const char* const qkv[3] = {"q", "k", "v"};
    static const char* const hn[2] = {"score", "weight"};
    // every tensor is looked up before anything is replaced
    for (const Vec& v : vecs)
        if (!tensor(v.name, v.floats)) return -2;
    for (const Lin& l : lins)
        if (!tensor(l.name, (size_t)l.rows * l.cols)) return -2;
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 2; ++t)
            for (const char* a : qkv)
                if (!tensor(fmt("maniqa.tab%d.%d.%s.weight", s + 1, t, a), (size_t)N * N) || !tensor(fmt("maniqa.tab%d.%d.%s.bias", s + 1, t, a), N)) return -2;
    for (const char* a : hn)
        if (!tensor(fmt("maniqa.%s.fc1.weight", a), (size_t)Eh * Eh) || !tensor(fmt("maniqa.%s.fc1.bias", a), Eh) || !tensor(fmt("maniqa.%s.fc2.weight", a), Eh) ||
            !tensor(fmt("maniqa.%s.fc2.bias", a), 1))
            return -2;

    std::vector<void*>& own = c->own[OWN_MANIQA];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[256];
    ir_maniqa_input_table_host(tab);
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m->tab)) return e;
    std::vector<float> t;
    for (const Vec& v : vecs)
        if (int e = own_copy(c, own, tensor(v.name, v.floats), v.floats * 4, hipMemcpyDeviceToDevice, v.dst)) return e;
    for (const Lin& l : lins) {
        t.assign((size_t)l.rows * l.cols, 0.f);
        if (int e = transposed_into(c, tensor(l.name, (size_t)l.rows * l.cols), l.rows, l.cols, t, l.rows, 0)) return e;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, l.dst)) return e;
    }
    // side by side: q | k | v of a TAB, fc1 of the two heads - one GEMM each, the same chain per output
    auto side_by_side = [&](const std::string& pre, const char* const* names, int count, const std::string& post, int rows, int cols, const float** w, const float** b) {
        t.assign((size_t)cols * count * rows, 0.f);
        std::vector<float> bias((size_t)count * rows);
        for (int k = 0; k < count; ++k) {
            const std::string base = pre + names[k] + post;
            if (int e = transposed_into(c, tensor(base + ".weight", (size_t)rows * cols), rows, cols, t, count * rows, k * rows)) return e;
            HIPOK(c, hipMemcpy(bias.data() + (size_t)k * rows, tensor(base + ".bias", rows), (size_t)rows * 4, hipMemcpyDeviceToHost));
        }
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, w)) return e;
        return own_copy(c, own, bias.data(), bias.size() * 4, hipMemcpyHostToDevice, b);
    };
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 2; ++k)
            if (int e = side_by_side(fmt("maniqa.tab%d.%d.", s + 1, k), qkv, 3, "", N, N, &m->tabw[s][k], &m->tabb[s][k])) return e;
    if (int e = side_by_side("maniqa.", hn, 2, ".fc1", Eh, Eh, &m->head_w1, &m->head_b1)) return e;
    std::vector<float> w2((size_t)2 * Eh), b2(2);
    for (int k = 0; k < 2; ++k) {
        HIPOK(c, hipMemcpy(w2.data() + (size_t)k * Eh, tensor(fmt("maniqa.%s.fc2.weight", hn[k]), Eh), (size_t)Eh * 4, hipMemcpyDeviceToHost));
        HIPOK(c, hipMemcpy(&b2[k], tensor(fmt("maniqa.%s.fc2.bias", hn[k]), 1), 4, hipMemcpyDeviceToHost));
    }
    if (int e = own_copy(c, own, w2.data(), w2.size() * 4, hipMemcpyHostToDevice, &m->head_w2)) return e;
    if (int e = own_copy(c, own, b2.data(), b2.size() * 4, hipMemcpyHostToDevice, &m->head_b2)) return e;
    m->ok = true;
    c->maniqa = *m;
    ++c->generation;
    return 0;
}

int ir_maniqa(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, const int* origins_yx, int crops, double* scores,
              float* feat, void* ws, size_t ws_bytes) {
    if (!c || !img || !scores || !ws || !origins_yx) return fail(c, -1, "ir_maniqa: null argument");
    if (crops < 1 || crops > IR_MANIQA_MAX_CROPS) return fail(c, -1, "ir_maniqa: %d crops (1 .. %d)", crops, IR_MANIQA_MAX_CROPS);
    if (int e = check_rect(c, "ir_maniqa", nullptr, n, h, w, 1, {{rows, pitch}})) return e;
    if (!c->maniqa.ok) return fail(c, -13, "ir_maniqa: MANIQA not configured (ir_maniqa_configure)");
    if (std::min(h, w) <= c->maniqa.crop) return fail(c, -1, "ir_maniqa: a %d x %d image has no %d x %d crops (the short side must be above it)", h, w, c->maniqa.crop, c->maniqa.crop);
    IrManiqaPlan pl;
    if (ir_maniqa_plan(c->maniqa, n, crops, 1, &pl)) return fail(c, -1, "ir_maniqa: n %d with %d crops is more than one call takes (4096 images)", n, crops);
    if (int e = check_ws(c, "ir_maniqa", ws, ws_bytes, pl.total, 256)) return e;
    if ((reinterpret_cast<uintptr_t>(scores) & 7) || (reinterpret_cast<uintptr_t>(feat) & 3) || (reinterpret_cast<uintptr_t>(origins_yx) & 3))
        return fail(c, -1, "ir_maniqa: scores / feat / origins not aligned");
    // as many crops per pass as the workspace holds: the plan's size grows with the pass, so the largest that fits is found by bisection
    int lo = 1, hi = (int)std::min<long>((long)n * crops, 32768);
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        IrManiqaPlan q;
        if (!ir_maniqa_plan(c->maniqa, n, crops, mid, &q) && q.total <= ws_bytes) lo = mid;
        else hi = mid - 1;
    }
    if (ir_maniqa_plan(c->maniqa, n, crops, lo, &pl) || pl.total > ws_bytes) return fail(c, -1, "ir_maniqa: no plan for %d crops per pass", lo);
    use_ctx(c);
    if (ir_launch_maniqa(c->maniqa, img, rows, pitch, n, h, w, origins_yx, crops, scores, feat, ws, pl, (hipStream_t)stream)) return fail(c, -100, "ir_maniqa: launch failed");
    return 0;
}

// ---------------------------------------------------------------- TOPIQ-NR (topiq.hip)
int ir_topiq_input_table(float* tab) {
    if (!tab) return -1;
    ir_topiq_input_table_host(tab);
    return 0;
}

int ir_topiq_configure(ir_ctx* c, const int* depths, int width, int dim, int heads, int ffn) {
    if (!c || !depths) return fail(c, -1, "ir_topiq_configure: null argument");
    int n_blocks = 0;
    for (int l = 0; l < 4; ++l) {
        if (depths[l] < 1) return fail(c, -1, "ir_topiq_configure: stage %d has %d blocks", l + 1, depths[l]);
        n_blocks += depths[l];
    }
    if (n_blocks > IR_TOPIQ_MAX_BLOCKS) return fail(c, -1, "ir_topiq_configure: %d blocks, at most %d", n_blocks, IR_TOPIQ_MAX_BLOCKS);
    if (width < 4 || width % 4 || width > 1024 || dim < 8 || dim % 8 || dim > IR_TOPIQ_MAX_DIM || heads < 1 || dim % heads || (dim / heads) % 4 || ffn < 4 || ffn % 4 ||
        ffn > 65536)
        return fail(c, -1, "ir_topiq_configure: unsupported model (width %d of 4, dim %d of 8 up to %d, %d heads of a multiple of 4, ffn %d of 4)", width, dim,
                    IR_TOPIQ_MAX_DIM, heads, ffn);
    HIPOK(c, hipSetDevice(c->device));
    c->topiq.ok = false;
    auto m = std::make_unique<IrTopiqModel>();
    for (int l = 0; l < 4; ++l) m->depths[l] = depths[l];
    m->width = width; m->dim = dim; m->heads = heads; m->ffn = ffn; m->n_blocks = n_blocks;
    const int D = dim, GHID = IR_TOPIQ_GATE_HIDDEN;
    struct Conv { std::string conv, bn; int cin, cout, ks, stride; IrTopiqConv* dst; };   // bn empty: conv + ".bias" is the shift
    struct Vec { std::string name; size_t floats; const float** dst; };                  // copied as it is
    struct Lin { std::string name; int rows, cols; const float** dst; };                 // [rows][cols] -> [cols][rows]
    std::vector<Conv> convs;
    std::vector<Vec> vecs;
    std::vector<Lin> lins;
    convs.push_back({"topiq.trunk.conv1", "topiq.trunk.bn1", 3, width, 7, 2, &m->stem});
    int inplanes = width, bi = 0;
    for (int l = 0; l < 4; ++l) {
        const int planes = width << l;
        for (int i = 0; i < depths[l]; ++i, ++bi) {
            IrTopiqBlock& b = m->blocks[bi];
            const int stride = (i == 0 && l > 0) ? 2 : 1;
            b.has_down = i == 0;
            const std::string base = fmt("topiq.trunk.layer%d.%d.", l + 1, i);
            convs.push_back({base + "conv1", base + "bn1", inplanes, planes, 1, 1, &b.c1});
            convs.push_back({base + "conv2", base + "bn2", planes, planes, 3, stride, &b.c2});
            convs.push_back({base + "conv3", base + "bn3", planes, planes * 4, 1, 1, &b.c3});
            if (b.has_down) convs.push_back({base + "downsample.0", base + "downsample.1", inplanes, planes * 4, 1, stride, &b.down});
            inplanes = planes * 4;
        }
    }
    auto attn = [&](const std::string& p, IrTopiqAttn& a, int norms) {
        const float** ng[3] = {&a.n1g, &a.n2g, &a.n3g};
        const float** nb[3] = {&a.n1b, &a.n2b, &a.n3b};
        for (int j = 0; j < norms; ++j) {
            vecs.push_back({fmt("%snorm%d.weight", p.c_str(), j + 1), (size_t)D, ng[j]});
            vecs.push_back({fmt("%snorm%d.bias", p.c_str(), j + 1), (size_t)D, nb[j]});
        }
        vecs.push_back({p + "attn.in_proj_bias", (size_t)3 * D, &a.inb});
        vecs.push_back({p + "attn.out_proj.bias", (size_t)D, &a.ob});
        vecs.push_back({p + "linear1.bias", (size_t)ffn, &a.f1b});
        vecs.push_back({p + "linear2.bias", (size_t)D, &a.f2b});
        lins.push_back({p + "attn.in_proj_weight", 3 * D, D, &a.inw});
        lins.push_back({p + "attn.out_proj.weight", D, D, &a.ow});
        lins.push_back({p + "linear1.weight", ffn, D, &a.f1w});
        lins.push_back({p + "linear2.weight", D, ffn, &a.f2w});
    };
    for (int i = 0; i < 5; ++i) {
        IrTopiqGate& g = m->gate[i];
        const int C = width << (i == 0 ? 0 : i + 1);
        const std::string p = fmt("topiq.gate.%d.", i);
        lins.push_back({p + "split.weight", 2 * C, C, &g.sw});
        vecs.push_back({p + "split.bias", (size_t)2 * C, &g.sb});
        lins.push_back({p + "conv1.weight", GHID, C, &g.w1});
        vecs.push_back({p + "conv1.bias", (size_t)GHID, &g.b1});
        convs.push_back({p + "conv2", "", GHID, GHID, 3, 1, &g.c2});
        vecs.push_back({p + "conv3.bias", 1, &g.b3});
        lins.push_back({fmt("topiq.reduce.%d.weight", i), D, C, &g.rw});
        vecs.push_back({fmt("topiq.reduce.%d.bias", i), (size_t)D, &g.rb});
        attn(fmt("topiq.sa.%d.", i), m->sa[i], 2);
    }
    for (int k = 0; k < 4; ++k) attn(fmt("topiq.ca.%d.", k), m->ca[k], 3);
    attn("topiq.pool.", m->pool, 2);
    static const int sidx[5] = {0, 1, 3, 4, 6};
    for (int j = 0; j < 5; ++j) {
        const size_t rows = sidx[j] == 6 ? 1 : D, cols = (sidx[j] == 0 || sidx[j] == 3) ? 1 : D;
        vecs.push_back({fmt("topiq.score.%d.weight", sidx[j]), rows * cols, &m->sc[2 * j]});
        vecs.push_back({fmt("topiq.score.%d.bias", sidx[j]), rows, &m->sc[2 * j + 1]});
    }
    vecs.push_back({"topiq.h_emb", (size_t)(D / 2) * IR_TOPIQ_EMB, &m->h_emb});
    vecs.push_back({"topiq.w_emb", (size_t)(D / 2) * IR_TOPIQ_EMB, &m->w_emb});

    auto tensor = [&](const std::string& name, size_t floats) { return exact_f32(c, "ir_topiq_configure", "the configured model's", name, floats); };
    static const char* const bnv[4] = {".weight", ".bias", ".running_mean", ".running_var"};
    // every tensor is looked up before anything is replaced
    for (const Conv& s : convs) {
        if (!tensor(s.conv + ".weight", (size_t)s.cout * s.cin * s.ks * s.ks)) return -2;
        if (s.bn.empty()) {
            if (!tensor(s.conv + ".bias", (size_t)s.cout)) return -2;
        } else {
            for (const char* v : bnv)
                if (!tensor(s.bn + v, (size_t)s.cout)) return -2;
        }
    }
    for (const Vec& v : vecs)
        if (!tensor(v.name, v.floats)) return -2;
    for (const Lin& l : lins)
        if (!tensor(l.name, (size_t)l.rows * l.cols)) return -2;
    for (int i = 0; i < 5; ++i)
        if (!tensor(fmt("topiq.gate.%d.conv3.weight", i), (size_t)9 * GHID)) return -2;

    std::vector<void*>& own = c->own[OWN_TOPIQ];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    float tab[3 * 256];
    ir_topiq_input_table_host(tab);
    if (int e = own_copy(c, own, tab, sizeof tab, hipMemcpyHostToDevice, &m->tab)) return e;
    std::vector<float> t;
    for (const Conv& s : convs) {   // the repacked weights, and BatchNorm folded in fp64
        if (int e = repacked_conv(c, tensor(s.conv + ".weight", (size_t)s.cout * s.cin * s.ks * s.ks), s.cin, s.cout, s.ks, t)) return e;
        s.dst->cin = s.cin; s.dst->cout = s.cout; s.dst->ks = s.ks; s.dst->stride = s.stride;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, &s.dst->w)) return e;
        if (s.bn.empty()) {
            if (int e = own_copy(c, own, tensor(s.conv + ".bias", (size_t)s.cout), (size_t)s.cout * 4, hipMemcpyDeviceToDevice, &s.dst->shift)) return e;
            continue;
        }
        std::vector<float> bn[4], sc(s.cout), sh(s.cout);
        for (int k = 0; k < 4; ++k) {
            bn[k].resize(s.cout);
            HIPOK(c, hipMemcpy(bn[k].data(), tensor(s.bn + bnv[k], (size_t)s.cout), (size_t)s.cout * 4, hipMemcpyDeviceToHost));
        }
        for (int o = 0; o < s.cout; ++o) {   // scale = g / sqrt(var + eps), shift = b - mean scale, each rounded to fp32 once
            const double scale = (double)bn[0][o] / sqrt((double)bn[3][o] + 1e-5);
            sc[o] = (float)scale;
            sh[o] = (float)((double)bn[1][o] - (double)bn[2][o] * scale);
        }
        if (int e = own_copy(c, own, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, &s.dst->scale)) return e;
        if (int e = own_copy(c, own, sh.data(), sh.size() * 4, hipMemcpyHostToDevice, &s.dst->shift)) return e;
    }
    for (const Vec& v : vecs)
        if (int e = own_copy(c, own, tensor(v.name, v.floats), v.floats * 4, hipMemcpyDeviceToDevice, v.dst)) return e;
    for (const Lin& l : lins) {
        t.assign((size_t)l.rows * l.cols, 0.f);
        if (int e = transposed_into(c, tensor(l.name, (size_t)l.rows * l.cols), l.rows, l.cols, t, l.rows, 0)) return e;
        if (int e = own_copy(c, own, t.data(), t.size() * 4, hipMemcpyHostToDevice, l.dst)) return e;
    }
    for (int i = 0; i < 5; ++i) {   // [1][64][3][3] -> [(ky, kx, c)]
        if (int e = repacked_conv(c, tensor(fmt("topiq.gate.%d.conv3.weight", i), (size_t)9 * GHID), GHID, 1, 3, t)) return e;
        if (int e = own_copy(c, own, t.data(), (size_t)9 * GHID * 4, hipMemcpyHostToDevice, &m->gate[i].w3)) return e;
    }
    m->ok = true;
    c->topiq = *m;
    ++c->generation;
    return 0;
}

int ir_topiq(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, float* level_means, void* ws,
             size_t ws_bytes) {
    if (!c || !img || !scores || !ws) return fail(c, -1, "ir_topiq: null argument");
    if (int e = check_rect(c, "ir_topiq", "the coarsest grid needs 16 x 16", n, h, w, IR_TOPIQ_MIN_EDGE, {{rows, pitch}})) return e;
    if (!c->topiq.ok) return fail(c, -13, "ir_topiq: TOPIQ not configured (ir_topiq_configure)");
    IrTopiqPlan pl;
    if (ir_topiq_plan(c->topiq, n, h, w, &pl)) return fail(c, -1, "ir_topiq: n %d of %d x %d is more than one call takes (2^31 output pixels, 65535 images)", n, h, w);
    if (int e = check_ws(c, "ir_topiq", ws, ws_bytes, pl.total, 256)) return e;
    if ((reinterpret_cast<uintptr_t>(scores) & 7) || (reinterpret_cast<uintptr_t>(feat) & 3) || (reinterpret_cast<uintptr_t>(level_means) & 3))
        return fail(c, -1, "ir_topiq: scores / feat / level_means not aligned");
    use_ctx(c);
    if (ir_launch_topiq(c->topiq, img, rows, pitch, n, h, w, scores, feat, level_means, ws, (hipStream_t)stream)) return fail(c, -100, "ir_topiq: launch failed");
    return 0;
}

// ---------------------------------------------------------------- NIQE's block statistics (niqe.hip)
// the half-size fp64 luma plane of every image's scored rectangle
static size_t niqe_workspace(int n, int h, int w) {
    const size_t H2 = (size_t)(h / IR_NIQE_BLOCK) * (IR_NIQE_BLOCK / 2), W2 = (size_t)(w / IR_NIQE_BLOCK) * (IR_NIQE_BLOCK / 2);
    return ((size_t)n * H2 * W2 * sizeof(double) + 255) & ~(size_t)255;
}
int ir_niqe_window(double* k49) {
    if (!k49) return -1;
    ir_niqe_window_host(k49);
    return 0;
}
int ir_niqe_stats(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* out, void* ws, size_t ws_bytes) {
    if (!c || !img || !out || !ws) return fail(c, -1, "ir_niqe_stats: null argument");
    if (int e = check_rect(c, "ir_niqe_stats", "a block is 96 x 96", n, h, w, IR_NIQE_BLOCK, {{rows, pitch}})) return e;
    if (int e = check_ws(c, "ir_niqe_stats", ws, ws_bytes, niqe_workspace(n, h, w), 8)) return e;
    if (int e = check_out8(c, "ir_niqe_stats", out)) return e;
    if (!c->niqe_tab) return fail(c, -1, "ir_niqe_stats: the context has no luma tables");
    use_ctx(c);
    if (ir_launch_niqe_stats(img, rows, pitch, n, h, w, c->niqe_tab, static_cast<double*>(ws), out, (hipStream_t)stream))
        return fail(c, -100, "ir_niqe_stats: launch failed (more than 65535 images or block rows)");
    return 0;
}

// ---------------------------------------------------------------- IL-NIQE's DFT and Weibull fit (ilniqe.hip)
// the column transform, real and imaginary
static size_t dft2_workspace(int size) { return size == 252 || size == 504 ? (size_t)2 * size * size * sizeof(double) : 0; }
// the double tensor `name` of the context with exactly `count` values, or null with ir_last_error naming it
static const double* exact_f64(ir_ctx* c, const char* who, const char* name, size_t count) {
    auto it = c->t.find(name);
    if (it == c->t.end() || it->second.bytes != count * 8) {
        fail(c, -2, "%s: tensor %s (%s; %zu doubles are needed)", who, name, it == c->t.end() ? "missing" : "another size", count);
        return nullptr;
    }
    return static_cast<const double*>(it->second.p);
}
int ir_ilniqe_plan_bytes(int h, int w) {
    if (h < 2 || w < 2) return -1;
    size_t a, b, d;
    const size_t bytes = ir_ilniqe_plan_layout(h, w, &a, &b, &d);
    return bytes > 0x7fffffff ? -1 : (int)bytes;
}
int ir_ilniqe_plan(int h, int w, void* host_tables, size_t bytes) {
    const int need = ir_ilniqe_plan_bytes(h, w);
    if (need < 0 || !host_tables || bytes < (size_t)need || (reinterpret_cast<uintptr_t>(host_tables) & 7)) return -1;
    ir_ilniqe_plan_host(h, w, host_tables);
    return 0;
}
int ir_ilniqe_configure(ir_ctx* c) {
    if (!c) return -1;
    HIPOK(c, hipSetDevice(c->device));
    c->ilniqe.ok = false;
    const char* const who = "ir_ilniqe_configure";
    static const int sizes[2] = {252, 504};
    const double *win5, *win6, *taps, *bank[2];   // every tensor is looked up before anything is replaced
    if (!(win5 = exact_f64(c, who, "ilniqe.win5", 25)) || !(win6 = exact_f64(c, who, "ilniqe.win6", 36)) || !(taps = exact_f64(c, who, "ilniqe.taps", 44)) ||
        !(bank[0] = exact_f64(c, who, "ilniqe.bank252", (size_t)12 * 252 * 252)) || !(bank[1] = exact_f64(c, who, "ilniqe.bank504", (size_t)12 * 504 * 504)))
        return -2;
    IrIlniqeTables m;
    std::vector<void*>& own = c->own[OWN_ILNIQE];
    release_list(own);
    HIPOK(c, hipDeviceSynchronize());
    HIPOK(c, hipMemcpy(m.win5, win5, sizeof m.win5, hipMemcpyDeviceToHost));
    HIPOK(c, hipMemcpy(m.win6, win6, sizeof m.win6, hipMemcpyDeviceToHost));
    HIPOK(c, hipMemcpy(m.taps, taps, sizeof m.taps, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k) {
        const size_t nn = (size_t)sizes[k] * sizes[k];
        std::vector<double> t(2 * nn);
        ir_ilniqe_twiddles_host(sizes[k], t.data(), t.data() + nn);
        void* d = nullptr;
        if (dev_alloc(c, own, &d, t.size() * sizeof(double))) return -100;
        HIPOK(c, hipMemcpy(d, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
        m.tw[k] = static_cast<const double*>(d);
        if (dev_alloc(c, own, &d, 12 * nn * sizeof(double))) return -100;
        HIPOK(c, hipMemcpy(d, bank[k], 12 * nn * sizeof(double), hipMemcpyDeviceToDevice));
        m.bank[k] = static_cast<const double*>(d);
    }
    m.ok = true;
    c->ilniqe = m;
    ++c->generation;
    return 0;
}
int ir_ilniqe_stats(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, const void* plan, double* out, void* ws,
                    size_t ws_bytes) {
    if (!c || !img || !plan || !out || !ws) return fail(c, -1, "ir_ilniqe_stats: null argument");
    if (int e = check_rect(c, "ir_ilniqe_stats", "an image is at least 2 x 2", n, h, w, 2, {{rows, pitch}})) return e;
    if (int e = check_ws(c, "ir_ilniqe_stats", ws, ws_bytes, ir_ilniqe_workspace(w), 8)) return e;
    if (int e = check_out8(c, "ir_ilniqe_stats", out)) return e;
    if (int e = check_out8(c, "ir_ilniqe_stats", plan)) return e;
    if (!c->ilniqe.ok) return fail(c, -1, "ir_ilniqe_stats: IL-NIQE's tables are not bound (ir_ilniqe_configure)");
    use_ctx(c);
    if (ir_launch_ilniqe_stats(c->ilniqe, img, rows, pitch, n, h, w, plan, out, static_cast<double*>(ws), (hipStream_t)stream))
        return fail(c, -100, "ir_ilniqe_stats: launch failed");
    return 0;
}
int ir_op_dft2_f64(ir_ctx* c, void* stream, const double* re, const double* im, int size, int inverse, double* out_re, double* out_im, void* ws,
                   size_t ws_bytes) {
    if (!c || !re || !out_re || !out_im || !ws) return fail(c, -1, "ir_op_dft2_f64: null argument");
    if (size != 252 && size != 504) return fail(c, -1, "ir_op_dft2_f64: bad size (%d; 252 or 504)", size);
    if (int e = check_ws(c, "ir_op_dft2_f64", ws, ws_bytes, dft2_workspace(size), 8)) return e;
    for (const void* p : {(const void*)re, (const void*)im, (const void*)out_re, (const void*)out_im})
        if (int e = check_out8(c, "ir_op_dft2_f64", p)) return e;
    const double* tw = c->ilniqe.ok ? c->ilniqe.tw[size == 504] : nullptr;
    if (!tw) return fail(c, -1, "ir_op_dft2_f64: IL-NIQE's tables are not bound (ir_ilniqe_configure)");
    use_ctx(c);
    if (ir_launch_dft2_f64(tw, tw + (size_t)size * size, re, im, size, inverse, out_re, out_im, static_cast<double*>(ws), (hipStream_t)stream))
        return fail(c, -100, "ir_op_dft2_f64: launch failed");
    return 0;
}
int ir_op_weibull_fit(ir_ctx* c, void* stream, const double* x, int rows, int count, double* k_lambda) {
    if (!c || !x || !k_lambda) return fail(c, -1, "ir_op_weibull_fit: null argument");
    if (rows < 1 || count < 2 || count > IR_WEIBULL_MAX) return fail(c, -1, "ir_op_weibull_fit: bad size (%d rows of %d; 2 .. %d values)", rows, count, IR_WEIBULL_MAX);
    if (int e = check_out8(c, "ir_op_weibull_fit", x)) return e;
    if (int e = check_out8(c, "ir_op_weibull_fit", k_lambda)) return e;
    use_ctx(c);
    if (ir_launch_weibull_fit(x, rows, count, k_lambda, (hipStream_t)stream)) return fail(c, -100, "ir_op_weibull_fit: launch failed");
    return 0;
}

// ---------------------------------------------------------------- low-quality inputs from ground truth (degrade.hip)
int ir_degrade_qtables(int q, uint16_t* luma64, uint16_t* chroma64) {
    if (!luma64 || !chroma64 || q < 1 || q > 100) return -1;
    ir_degrade_qtables_host(q, luma64, chroma64);
    return 0;
}
int ir_degrade(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, const ir_degrade_params* params, uint8_t* out,
               uint8_t* jpeg_or_null, void* ws, size_t ws_bytes) {
    if (!c || !img || !params || !out || !ws) return fail(c, -1, "ir_degrade: null argument");
    if (int e = check_rect(c, "ir_degrade", nullptr, n, h, w, 1, {{rows, pitch}}, (long)h * w > (1L << 28))) return e;
    for (int i = 0; i < n; ++i) {   // every image is checked before the first launch
        const ir_degrade_params& p = params[i];
        if (!p.kernel) return fail(c, -1, "ir_degrade: image %d has no blur kernel", i);
        if (p.ksize < 1 || p.ksize > IR_DEGRADE_MAX_KSIZE || !(p.ksize & 1))
            return fail(c, -1, "ir_degrade: image %d: the blur kernel size %d is not odd and within 1 .. %d", i, p.ksize, IR_DEGRADE_MAX_KSIZE);
        if (h < p.ksize / 2 + 1 || w < p.ksize / 2 + 1)
            return fail(c, -1, "ir_degrade: a %d x %d image is too small for a %d x %d blur (reflection needs %d pixels)", h, w, p.ksize, p.ksize, p.ksize / 2 + 1);
        if (p.lh < IR_DEGRADE_MIN_LOW || p.lw < IR_DEGRADE_MIN_LOW || p.lh > h || p.lw > w)
            return fail(c, -1, "ir_degrade: image %d: low-resolution size %d x %d outside %d .. %d x %d", i, p.lh, p.lw, IR_DEGRADE_MIN_LOW, h, w);
        if (p.q < 0 || p.q > 100) return fail(c, -1, "ir_degrade: image %d: JPEG quality %d outside 0 .. 100", i, p.q);
        if (p.norm != IR_DEGRADE_NORM_NONE && p.norm != IR_DEGRADE_NORM_MAX) return fail(c, -1, "ir_degrade: image %d: unknown norm %d", i, p.norm);
        if ((reinterpret_cast<uintptr_t>(p.kernel) & 7) || (reinterpret_cast<uintptr_t>(p.noise) & 3))
            return fail(c, -1, "ir_degrade: image %d: misaligned kernel or noise pointer", i);
    }
    if (int e = check_ws(c, "ir_degrade", ws, ws_bytes, ir_degrade_workspace(h, w), 256)) return e;
    use_ctx(c);
    for (int i = 0; i < n; ++i) {
        const ir_degrade_params& p = params[i];
        if (ir_launch_degrade(img + (long)i * rows * pitch, pitch, h, w, p.kernel, p.ksize, p.lh, p.lw, p.sigma, p.q, p.noise, p.norm,
                              out + (long)i * rows * pitch, pitch, jpeg_or_null ? jpeg_or_null + (long)i * h * w * 3 : nullptr, ws, (hipStream_t)stream))
            return fail(c, -100, "ir_degrade: launch failed (image %d)", i);
    }
    return 0;
}

// ---------------------------------------------------------------- the second-order degradation chain (degrade_chain.hip)
static long chain_tap_floats(const ir_chain& ch, int h, int w) {   // the size of the image behind op `tap`
    if (ch.tap < 0) return 0;
    for (int i = 0; i <= ch.tap; ++i)
        if (ch.ops[i].kind == IR_CHAIN_RESIZE) h = ch.ops[i].b, w = ch.ops[i].c;
    return (long)h * w * 3;
}
int ir_degrade_chain(ir_ctx* c, void* stream, const uint8_t* img, int rows, long pitch, int n, int h, int w, const ir_chain* chains, uint8_t* out,
                     float* tap_or_null, void* ws, size_t ws_bytes) {
    if (!c || !img || !chains || !out || !ws) return fail(c, -1, "ir_degrade_chain: null argument");
    if (int e = check_rect(c, "ir_degrade_chain", nullptr, n, h, w, 1, {{rows, pitch}}, h > IR_CHAIN_MAX_SIDE || w > IR_CHAIN_MAX_SIDE)) return e;
    int mh = h, mw = w;
    for (int i = 0; i < n; ++i) {   // every chain is checked before the first launch
        int ih, iw;
        const char* why;
        if (ir_degrade_chain_check(&chains[i], h, w, &ih, &iw, &why)) return fail(c, -1, "ir_degrade_chain: image %d (%d x %d): %s", i, h, w, why);
        mh = std::max(mh, ih), mw = std::max(mw, iw);
    }
    if (int e = check_ws(c, "ir_degrade_chain", ws, ws_bytes, ir_degrade_chain_workspace(h, w, mh, mw), 256)) return e;
    if (tap_or_null && (reinterpret_cast<uintptr_t>(tap_or_null) & 3)) return fail(c, -1, "ir_degrade_chain: misaligned tap pointer");
    use_ctx(c);
    for (int i = 0; i < n; ++i) {
        if (ir_launch_degrade_chain(img + (long)i * rows * pitch, pitch, h, w, &chains[i], mh, mw, out + (long)i * rows * pitch, pitch, tap_or_null, ws,
                                    (hipStream_t)stream))
            return fail(c, -100, "ir_degrade_chain: launch failed (image %d)", i);
        if (tap_or_null) tap_or_null += chain_tap_floats(chains[i], h, w);
    }
    return 0;
}
}  // extern "C"

// the tables ir_init gives every context (both in OWN_CTX)
int ir_host::image_init(ir_ctx* c) {
    auto upload = [c](const double* tab, size_t bytes, double** out) {
        if (dev_alloc(c, c->own[OWN_CTX], reinterpret_cast<void**>(out), bytes)) return -100;
        HIPOK(c, hipMemcpy(*out, tab, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    double tab[4 * 256];
    // ir_metrics_y's luma tables: c_k * (double)((float)v / 255.0f), the float32 division of the host model done once on the host
    static const double bt601[3] = {65.481, 128.553, 24.966};
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < 256; ++v) {
            volatile float x = (float)v / 255.0f;
            tab[256 * k + v] = bt601[k] * (double)x;
        }
    if (int e = upload(tab, 3 * 256 * sizeof(double), &c->luma_tab)) return e;
    // ir_niqe_stats' tables: the YIQ luma terms coef_c * (double)((float)v / 255.0f), then v / 255.0 (the unit scale the half-size filter works on)
    static const double yiq[3] = {0.299, 0.587, 0.114};
    for (int v = 0; v < 256; ++v) {
        volatile float x = (float)v / 255.0f;
        for (int k = 0; k < 3; ++k) tab[256 * k + v] = yiq[k] * (double)x;
        tab[768 + v] = (double)v / 255.0;
    }
    return upload(tab, sizeof tab, &c->niqe_tab);
}

// Sizes alone decide every answer except CLIP-IQA's, MUSIQ's, MANIQA's and TOPIQ's, which also take the configured model's shape: no context is needed for the others.
bool ir_host::image_workspace(ir_ctx* c, int stage, int n, int h, int w, int flags, int tile_size, size_t* bytes) {
    const bool some = n >= 1 && h >= 1 && w >= 1;
    IrClipiqaPlan cp;
    IrMusiqPlan mp;
    IrManiqaPlan qp;
    IrTopiqPlan tp;
    IrLpipsPlan lp;
    IrDistsPlan dp;
    IrFidPlan fp;
    IrJpegLayout jl;
    *bytes = 0;
    switch (stage) {
        case IR_STAGE_DEGRADE_CHAIN: if (n >= 1) *bytes = ir_degrade_chain_workspace(h, w, flags, tile_size); break;   // flags, tile_size: the largest intermediate image
        case IR_STAGE_DEGRADE: if (n >= 1) *bytes = ir_degrade_workspace(h, w); break;   // the images of a batch share it
        case IR_STAGE_NIQE: if (n >= 1 && h >= IR_NIQE_BLOCK && w >= IR_NIQE_BLOCK) *bytes = niqe_workspace(n, h, w); break;
        case IR_STAGE_ILNIQE: if (n >= 1 && h >= 2 && w >= 2) *bytes = ir_ilniqe_workspace(w); break;   // the images of a batch share it
        case IR_STAGE_ILNIQE_DFT: if (n >= 1 && h == w) *bytes = dft2_workspace(h); break;
        case IR_STAGE_CLIPIQA: if (c && c->clipiqa.ok && !ir_clipiqa_plan(c->clipiqa, n, h, w, &cp)) *bytes = cp.total; break;
        case IR_STAGE_MUSIQ: if (c && c->musiq.ok && !ir_musiq_plan(c->musiq, n, h, w, &mp)) *bytes = mp.total; break;
        case IR_STAGE_MANIQA:   // flags: the crops per image, tile_size: the crops per pass (0: one, the least a call takes); h and w do not matter
            if (c && c->maniqa.ok && !ir_maniqa_plan(c->maniqa, n, flags, std::max(tile_size, 1), &qp)) *bytes = qp.total;
            break;
        case IR_STAGE_TOPIQ: if (c && c->topiq.ok && !ir_topiq_plan(c->topiq, n, h, w, &tp)) *bytes = tp.total; break;
        case IR_STAGE_LPIPS: if (!ir_lpips_plan(n, h, w, &lp)) *bytes = lp.total; break;
        case IR_STAGE_DISTS: if (!ir_dists_plan(n, h, w, &dp)) *bytes = dp.total; break;
        case IR_STAGE_FID: if (!ir_fid_plan(n, &fp)) *bytes = fp.total; break;
        case IR_STAGE_METRICS: if (some) *bytes = metrics_workspace(n, h, w); break;
        case IR_STAGE_JPEG: if (ir_jpeg_layout(n, h, w, flags, tile_size, &jl)) *bytes = jl.total; break;   // flags: the subsampling, tile_size: restart_mcus
        case IR_STAGE_JPEG_DECODE: if (n >= 1) *bytes = ir_jpeg_decode_workspace(h, w, (uint32_t)flags, tile_size); break;   // flags: stream_bytes, tile_size: subseq_bits
        case IR_STAGE_PNG_DECODE: if (n >= 1) *bytes = ir_png_decode_workspace(h, w, (uint32_t)flags, tile_size); break;   // flags: stream_bytes, tile_size: span_bits
        case IR_STAGE_PNG: if (some) *bytes = png_layout(n, h, w).total; break;
        case IR_STAGE_PNG_RUNS: if (some) *bytes = png_runs_layout(n, h, w).total; break;
        case IR_STAGE_RESAMPLE: if (some) *bytes = rs_workspace(n, h, w); break;   // n images, h = in_h, w = out_w: the uint8 image between the passes
        default: return false;
    }
    return true;
}
