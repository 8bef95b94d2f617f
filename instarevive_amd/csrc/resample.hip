// Pillow's 8-bit separable resampling (Resample.c) of uint8 HWC RGB device images (ir_resample_u8): horizontal pass, then vertical pass, the
// image between them uint8 (rounded and clipped like the final one), a pass whose input and output length are equal skipped. The bounds and
// coefficient tables come from the host (ir_resample_plan: they need double sin(), which the device would not reproduce bit for bit); per
// output sample the arithmetic is ss = 2^21 + sum(pixel * k) in int32, out = clamp(ss >> 22, 0, 255), so the result is Pillow's, bit for bit.
// Two launches through a uint8 intermediate [n][in_h][inter_pitch] in the caller's workspace (one launch when a pass is skipped, a padded
// copy when both are). A one-launch form - a 64 x 64 output tile per workgroup, the horizontal pass of the ~22 source rows it reaches kept
// in LDS with the tile's coefficients - was built and timed against this one: 0.031 against 0.033 ms for 512 x 512 -> 2048 x 2048 bicubic,
// 0.114 against 0.113 ms for 2048 x 2048 -> 1500 x 1500 LANCZOS, beside a 115.8 ms network step (profiles/resample.txt). It bought nothing,
// needed this form anyway for strong reductions (LANCZOS 2048 -> 97: 129 coefficients per sample, hundreds of source rows per tile), and
// was removed. A lane produces four consecutive bytes of an output row - the dword it stores - so a vertical lane shares one bounds
// entry and coefficient row over its four sums and loads whole dwords of the intermediate. The second launch also zero-fills the
// destination's padding (rows out_h .. full_h, columns out_w .. full_w): the pad to multiples of 64 of the network input.
// ir_resample_u8_window runs the same passes for a window of the result alone (the centre crop's last step): the horizontal pass makes the
// window's columns of the source rows the window's vertical taps reach - it reads that span from the plan's vertical bounds - and the
// vertical pass the window's rows; a skipped pass copies from the window's first row / byte, which is on a dword boundary only by chance,
// so the dword loads fall back to bytes there.
// Every launch first compares the plan's header with the call's sizes and writes nothing when they differ; the table entries are clipped to
// the source extent before they index it, so a damaged plan cannot make a lane read or write outside the buffers.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int TPB = 256;
constexpr int PRECISION_BITS = 22;

struct Pass {
    const uint8_t* src;   // image 0, row 0
    long src_pitch, src_img;
    int src_len;          // extent of the source along the pass's axis (what the bounds are clipped to)
    int src_dwords;       // rows of the source may be read as whole dwords up to byte src_cap
    int src_cap;
    uint8_t* dst;
    long dst_pitch, dst_img;
    int dst_dwords;       // rows of the destination start on dword boundaries
    int valid_h, valid_bytes;   // rows / bytes per row that hold samples
    int rows, row_bytes;        // rows / bytes per row that are written (the rest, beyond the samples: zeros)
    const int* plan;
    int in_h, in_w, out_h, out_w;   // of the whole call: what the plan's header must say
    // the window form alone (ir_resample_u8_window; zeros otherwise): the pass produces columns x_org .. / rows y_org .. of its virtual result
    int x_org, y_org;
    int span_rows;        // horizontal pass ahead of a vertical one: rows y_org .. y_org + span_rows of the result decide which source rows it covers
};

IR_DEVINL uint32_t clip8(int ss) {
    const int v = ss >> PRECISION_BITS;   // arithmetic shift, as Pillow's
    return (uint32_t)min(max(v, 0), 255);
}

// MODE 0: horizontal pass, 1: vertical pass, 2: copy (both passes skipped). WIN: the window form - the table index of an output sample is its
// place in the window plus the pass's origin (without WIN the origins are the constant 0 and the code is the whole-image one); the caller
// has moved the source pointer to the window's first row / byte where the pass copies that axis.
template <int MODE, bool WIN>
__global__ __launch_bounds__(TPB) void resample_pass_kernel(Pass p) {
    const int* hd = p.plan;
    if (hd[0] != IR_RESAMPLE_MAGIC || hd[1] != p.in_h || hd[2] != p.in_w || hd[3] != p.out_h || hd[4] != p.out_w) return;
    const int yy = blockIdx.y, image = blockIdx.z;
    const int j0 = 4 * (blockIdx.x * TPB + threadIdx.x);
    if (j0 >= p.row_bytes || yy >= p.rows) return;
    const int x_org = WIN ? p.x_org : 0, y_org = WIN ? p.y_org : 0;
    if (WIN && MODE == 0 && p.span_rows > 0) {
        // only the source rows the window's vertical taps reach (the bounds ascend with the row): first row's start .. last row's end,
        // clipped like every table entry; the vertical pass reads no other row of the intermediate
        const int ksv = hd[7];
        const int* vb = hd + hd[10];
        const int last = y_org + p.span_rows - 1;
        const int lo = min(max(vb[2 * y_org], 0), p.in_h);
        const int lmin = min(max(vb[2 * last], 0), p.in_h);
        const int hi = lmin + min(min(vb[2 * last + 1], ksv), p.in_h - lmin);
        if (yy < lo || yy >= hi) return;
    }
    uint32_t v = 0;
    if (yy < p.valid_h && j0 < p.valid_bytes) {
        const uint8_t* simg = p.src + (long)image * p.src_img;
        if (MODE == 0) {
            const int ks = hd[6];
            const int* bounds = hd + hd[8];
            const int* kk = hd + hd[9];
            const uint8_t* srow = simg + (long)yy * p.src_pitch;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = j0 + b;
                if (j < p.valid_bytes) {
                    const int xw = j / 3, c = j - 3 * xw, xx = xw + x_org;
                    const int xmin = min(max(bounds[2 * xx], 0), p.src_len);
                    const int xmax = min(min(bounds[2 * xx + 1], ks), p.src_len - xmin);
                    const int* k = kk + (long)xx * ks;
                    const uint8_t* q = srow + 3 * xmin + c;
                    int ss = 1 << (PRECISION_BITS - 1);
                    for (int x = 0; x < xmax; ++x) ss += (int)q[3 * x] * k[x];
                    v |= clip8(ss) << (8 * b);
                }
            }
        } else {
            int ymin = yy, ymax = 1, ks = 0;
            const int* k = nullptr;
            if (MODE == 1) {
                ks = hd[7];
                const int* bounds = hd + hd[10];
                const int yt = yy + y_org;
                ymin = min(max(bounds[2 * yt], 0), p.src_len);
                ymax = min(min(bounds[2 * yt + 1], ks), p.src_len - ymin);
                k = hd + hd[11] + (long)yt * ks;
            }
            const int half = MODE == 1 ? 1 << (PRECISION_BITS - 1) : 0;
            int s0 = half, s1 = half, s2 = half, s3 = half;
            const uint8_t* q = simg + (long)ymin * p.src_pitch + j0;
            if (p.src_dwords && j0 + 4 <= p.src_cap) {
                for (int y = 0; y < ymax; ++y) {
                    const uint32_t d = *reinterpret_cast<const uint32_t*>(q + (long)y * p.src_pitch);
                    const int c = MODE == 1 ? k[y] : 1;
                    s0 += (int)(d & 255) * c;
                    s1 += (int)((d >> 8) & 255) * c;
                    s2 += (int)((d >> 16) & 255) * c;
                    s3 += (int)(d >> 24) * c;
                }
            } else {
                const int left = p.valid_bytes - j0;   // >= 1
                for (int y = 0; y < ymax; ++y) {
                    const uint8_t* r = q + (long)y * p.src_pitch;
                    const int c = MODE == 1 ? k[y] : 1;
                    s0 += (int)r[0] * c;
                    if (left > 1) s1 += (int)r[1] * c;
                    if (left > 2) s2 += (int)r[2] * c;
                    if (left > 3) s3 += (int)r[3] * c;
                }
            }
            if (MODE == 1) {
                v = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16) | (clip8(s3) << 24);
            } else {
                v = (uint32_t)s0 | ((uint32_t)s1 << 8) | ((uint32_t)s2 << 16) | ((uint32_t)s3 << 24);
            }
            const int left = p.valid_bytes - j0;
            if (left < 4) v &= (1u << (8 * left)) - 1u;   // bytes behind the last sample belong to the padding
        }
    }
    uint8_t* drow = p.dst + (long)image * p.dst_img + (long)yy * p.dst_pitch;
    if (p.dst_dwords && j0 + 4 <= p.row_bytes) {
        *reinterpret_cast<uint32_t*>(drow + j0) = v;
    } else {
        for (int b = 0; b < 4 && j0 + b < p.row_bytes; ++b) drow[j0 + b] = (uint8_t)(v >> (8 * b));
    }
}

template <int MODE, bool WIN = false>
void launch_pass(const Pass& p, int n, hipStream_t s) {
    const dim3 grid(((p.row_bytes + 3) / 4 + TPB - 1) / TPB, p.rows, n);
    hipLaunchKernelGGL((resample_pass_kernel<MODE, WIN>), grid, dim3(TPB), 0, s, p);
}

inline int dword_aligned(const void* ptr, long pitch, long img) { return ((reinterpret_cast<uintptr_t>(ptr) | (uintptr_t)pitch | (uintptr_t)img) & 3) == 0; }

}  // namespace

int ir_launch_resample_u8(const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int full_h, int full_w,
                          long out_pitch, const int* plan, uint8_t* inter, long inter_pitch, hipStream_t s) {
    if (n > 65535 || in_h > 65535 || full_h > 65535) return -1;   // grid.y / grid.z
    const bool need_h = in_w != out_w, need_v = in_h != out_h;
    Pass p{};
    p.plan = plan;
    p.in_h = in_h; p.in_w = in_w; p.out_h = out_h; p.out_w = out_w;
    // the source side of the first launch and the destination side of the last are the caller's buffers
    Pass first = p, last = p;
    first.src = in; first.src_pitch = in_pitch; first.src_img = (long)in_h * in_pitch;
    first.src_dwords = dword_aligned(in, in_pitch, first.src_img); first.src_cap = 3 * in_w;
    last.dst = out; last.dst_pitch = out_pitch; last.dst_img = (long)full_h * out_pitch;
    last.dst_dwords = dword_aligned(out, out_pitch, last.dst_img);
    last.valid_h = out_h; last.valid_bytes = 3 * out_w; last.rows = full_h; last.row_bytes = 3 * full_w;
    if (need_h && need_v) {
        first.src_len = in_w;
        first.dst = inter; first.dst_pitch = inter_pitch; first.dst_img = (long)in_h * inter_pitch; first.dst_dwords = 1;
        first.valid_h = in_h; first.valid_bytes = 3 * out_w; first.rows = in_h; first.row_bytes = (int)inter_pitch;
        last.src = inter; last.src_pitch = inter_pitch; last.src_img = first.dst_img; last.src_dwords = 1; last.src_cap = (int)inter_pitch;
        last.src_len = in_h;
        launch_pass<0>(first, n, s);
        launch_pass<1>(last, n, s);
    } else {
        last.src = first.src; last.src_pitch = first.src_pitch; last.src_img = first.src_img; last.src_dwords = first.src_dwords; last.src_cap = first.src_cap;
        last.src_len = need_h ? in_w : in_h;
        if (need_h) launch_pass<0>(last, n, s);
        else if (need_v) launch_pass<1>(last, n, s);
        else launch_pass<2>(last, n, s);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The window form: rows y0 .. y0 + win_h, columns x0 .. x0 + win_w of the virtual out_h x out_w result, into the top-left corner of out.
// The intermediate is [n][in_h][inter_pitch] with win_w samples per row; the horizontal pass fills only the rows the vertical taps of the window reach.
int ir_launch_resample_u8_window(const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int y0, int x0, int win_h,
                                 int win_w, int full_h, int full_w, long out_pitch, const int* plan, uint8_t* inter, long inter_pitch, hipStream_t s) {
    if (n > 65535 || in_h > 65535 || full_h > 65535) return -1;   // grid.y / grid.z
    const bool need_h = in_w != out_w, need_v = in_h != out_h;
    Pass p{};
    p.plan = plan;
    p.in_h = in_h; p.in_w = in_w; p.out_h = out_h; p.out_w = out_w;
    Pass first = p, last = p;
    const long in_img = (long)in_h * in_pitch;
    last.dst = out; last.dst_pitch = out_pitch; last.dst_img = (long)full_h * out_pitch;
    last.dst_dwords = dword_aligned(out, out_pitch, last.dst_img);
    last.valid_h = win_h; last.valid_bytes = 3 * win_w; last.rows = full_h; last.row_bytes = 3 * full_w;
    if (need_h && need_v) {
        first.src = in; first.src_pitch = in_pitch; first.src_img = in_img; first.src_len = in_w;
        first.dst = inter; first.dst_pitch = inter_pitch; first.dst_img = (long)in_h * inter_pitch; first.dst_dwords = 1;
        first.valid_h = in_h; first.valid_bytes = 3 * win_w; first.rows = in_h; first.row_bytes = (int)inter_pitch;
        first.x_org = x0; first.y_org = y0; first.span_rows = win_h;
        last.src = inter; last.src_pitch = inter_pitch; last.src_img = first.dst_img; last.src_dwords = 1; last.src_cap = (int)inter_pitch;
        last.src_len = in_h; last.y_org = y0;
        launch_pass<0, true>(first, n, s);
        launch_pass<1, true>(last, n, s);
    } else if (need_h) {   // the rows are copied: the source starts at the window's first row
        last.src = in + (long)y0 * in_pitch; last.src_pitch = in_pitch; last.src_img = in_img; last.src_len = in_w; last.x_org = x0;
        launch_pass<0, true>(last, n, s);
    } else {   // the columns are copied: the source starts at the window's first byte, which is on a dword boundary only by chance
        last.src = in + 3L * x0 + (need_v ? 0 : (long)y0 * in_pitch); last.src_pitch = in_pitch; last.src_img = in_img;
        last.src_dwords = dword_aligned(last.src, in_pitch, in_img); last.src_cap = 3 * (in_w - x0);
        last.src_len = in_h; last.y_org = y0;
        if (need_v) launch_pass<1, true>(last, n, s);
        else launch_pass<2, true>(last, n, s);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
