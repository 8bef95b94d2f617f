// Internal launcher interface between the C-ABI layer (api.cpp, api_image.cpp) and the HIP kernels. Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_t;

// 1: launchers pick the older 4-wave kernels only (ir_set_plain_kernels; defined in igemm.hip)
extern int g_ir_plain_kernels;

// ---- implicit GEMM (igemm.hip)
struct IGemmParams {
    // A operand: NHWC bf16 activations. taps==1: row m at in + m*in_cs. taps==9: 3x3 window around output pixel.
    const bf16_t* in;
    int NB, H, W;   // input batch / height / width (before the optional nearest-2x upsample)
    int Cin;        // channels reduced over per tap (multiple of 32; zero-padded channels are fine)
    int in_cs;      // elements between consecutive pixels / rows of `in`
    int Ho, Wo;     // output height / width
    int taps;       // 1 or 9
    int stride;     // 1 or 2
    int pad;        // 1: symmetric "same" pad; 0: pad only bottom/right (the VAE's (0,1,0,1) stride-2 downsample)
    int up;         // 1: conv runs on the nearest-2x upsampled input (2H x 2W), folded into addressing
    // B operand
    const bf16_t* wgt;  // [Cout_pad][taps*Cin] bf16, K contiguous; rows wgt_rs elements apart
    long wgt_rs;
    int Cout, Cout_pad, M;
    // epilogue: v = act(acc + bias) * out_scale; v *= gate; v += res; store
    const float* bias;  // [Cout_pad] or null
    int act;
    float slope;
    float out_scale;
    const float* gate;  // gate[(m / rows_per_batch) * gate_stride + n] or null
    int gate_stride, rows_per_batch;
    const void* res;    // residual [.][res_cs], row index m (or m % res_mod when res_mod > 0)
    int res_f32, res_cs, res_mod;
    void* out;
    int out_f32, out_cs;
    bf16_t* out2;       // optional extra bf16 copy of the result
    int out2_cs;
    int fp8;            // 1: `in` and `wgt` hold OCP e4m3 bytes; Cin / in_cs / wgt_rs count PAIRS of fp8 channels (2-byte units), gate
                        // carries the dequantisation factor per output channel, bias is pre-divided by it (3x3 stride-1 convs only)
    int force_generic;  // 1: never take the halo-tile conv path (A/B testing)
    int vec;            // set by the launcher: all strides/pointers allow 4-element vector I/O
    // Optional fused GroupNorm statistics of the OUTPUT (the tensor a following GroupNorm normalises): every workgroup writes
    // the per-group sum and sum of squares of its (bf16-rounded) outputs to gn_part[((image*gn_chunks + chunk)*2 + {0,1})*G + g],
    // G = Cout / gn_cpg, chunk = the workgroup's pixel tile within the image. Set gn_chunks from ir_igemm_gn_chunks().
    float* gn_part;
    int gn_cpg, gn_chunks;
    // Split-K for small-M launches: the caller sets allow_splitk and, when ir_igemm_splitk(p) > 1, ks_ws (that many slices of p.M * Cout_pad
    // floats of scratch); ksplit is set by the launcher. Each split stores its partial tile in its own slice; a second kernel adds the
    // slices in order and applies the epilogue (deterministic). item_rows (0: M): the output rows of ONE batch item; the split count comes
    // from one item's tiles, so that an item sums in the same order in a batch as alone (whether a launch splits at all is still a matter of
    // the whole launch's tile count).
    int allow_splitk, ksplit, item_rows;
    int s1_min_tiles;   // > 32: conv_halo_s1_kernel only takes images with at least that many patch tiles (callers that never batch small images)
    float* ks_ws;
    // Optional second, TRANSPOSED copy of the output columns >= vt_col0 (gemm_pp_kernel's bf16 form only; M % 256 == 0, vt_T % 64 == 0): column
    // vt_col0 + head * vt_hd + d of row m = batch * vt_T + t goes to vt_out[batch * vt_bs + (head * vt_dv + d) * vt_ld + t] - the V^T operand of
    // the DiT self-attention straight from the qkv projection's epilogue (the rows d >= vt_hd of a head - the ones row and the padding - are
    // written once per run by ir_launch_vt_pad_init). ir_igemm_writes_vt(p) tells whether the launch ir_launch_igemm picks honours it.
    bf16_t* vt_out;
    int vt_col0, vt_hd, vt_dv, vt_ld, vt_T;
    long vt_bs;
    // 1: `wgt` holds the four sub-pixel phase matrices [2 dy + dx][Cout_pad][2 sy + sx][Cin] of an up = 1 conv (wgt_rs = 4 * Cin): only valid when
    // ir_conv_s1_up2x2_takes(p) - the caller asks first and passes the ordinary 9-tap weights otherwise
    int up2x2;
    // GroupNorm + SiLU of the INPUT applied inside conv_halo_s1_kernel (NORM form): per image and input channel scale / shift ([NB][Cin] fp32, what
    // ir_launch_groupnorm_fused(..., y = nullptr) leaves in its workspace); `in` is then the un-normalised tensor. Only when ir_conv_s1_norm_takes(p).
    const float* nrm_scale;
    const float* nrm_shift;
};
bool ir_conv_s1_norm_takes(const IGemmParams& p);
int ir_igemm_writes_vt(const IGemmParams& p);
int ir_launch_vt_pad_init(bf16_t* vt, int heads_total, int D, int DV, int T, int Tpad, hipStream_t s);
struct IGemmRoute;
// route: what ir_igemm_route(p) returned for this very p (a caller that asked for its profiler row passes it on), or null
int ir_launch_igemm(const IGemmParams& p, hipStream_t s, const IGemmRoute* route = nullptr);
// which kernel ir_launch_igemm picks for p: 0 conv_halo_s1, 1 conv_halo_pp, 2 gemm_pp, 3 conv_halo, 4 igemm_kernel (profiler rows)
int ir_igemm_kernel_id(const IGemmParams& p);
// The whole choice ir_launch_igemm makes for p, made in ONE place (ir_igemm_route): the launcher dispatches on it, ir_igemm_kernel_id is its
// `kernel` field and ir_op_igemm_route reports it to the tests.
struct IGemmRoute {
    int kernel;   // ir_igemm_kernel_id's value (5: conv64_kernel)
    int form;     // gemm_pp_kernel: 0 <NONE, 0, unit>, 1 <GELU_TANH, 0, unit>, 2 <NONE, 1>, 3 the general <-1, -1>; the conv kernels: 0 plain,
                  // 1 nearest-2x folded in, 2 sub-pixel phase weights, 3 (conv_halo_s1 only) the NORM form; igemm_kernel: 0
    int bn;       // output columns per tile (conv_halo_s1 / conv64: 0, their own files decide)
    int bk, stages, waves;   // igemm_kernel: BK (64 / 32), ring of 2 / 4 k-tiles (NST), 4 / 8 waves; 0 for the other kernels
    int taps;
    int splits;   // split-K slices (0: none); > 1 only with kernel 4, followed by splitk_finish_kernel
    int padded;   // tile order of tile_of_block: 1 XCD-padded (grid = row tiles rounded up to 8, times column tiles), 0 one block per tile
    int idle;     // 1: a padded grid that has blocks without a tile
    int fp8;
    int vt;       // 1: the launch writes IGemmParams::vt_out itself (ir_igemm_writes_vt: gemm_pp_kernel's bf16 form on whole tiles); the launcher
                  // hands vt_out to no other kernel
};
IGemmRoute ir_igemm_route(const IGemmParams& p);
// bits 0-3 kernel, 4-6 form, 7 vt, 8-15 bn / 4, 16-19 bk / 16, 20-23 stages, 24-27 waves, 28-31 taps, 32-39 splits, 40 padded, 41 idle, 42 fp8
long long ir_igemm_route_pack(const IGemmRoute& r);
// The range of ir_igemm_route for bf16 operands, taken from the rule itself: the distinct packed routes - splits, padded, idle and vt cleared -
// it returns over a grid of launches that crosses every threshold it reads (taps, Cin, Cout_pad, rows / map size, stride, upsample forms,
// epilogue forms, split-K, plain kernels). -> their number; the first min(number, cap) in out. No device is touched.
int ir_igemm_route_range(long long* out, int cap);
// Pixel tiles per image the kernel ir_launch_igemm would pick for p writes statistics for, or 0 if this launch cannot fuse them.
int ir_igemm_gn_chunks(const IGemmParams& p);
// Split count ir_launch_igemm would use for p given a workspace (0: none); see IGemmParams::allow_splitk.
int ir_igemm_splitk(const IGemmParams& p);

// conv_s1.hip: the one-wave-per-SIMD 3x3 convolution (16 x 32 patches x 128 channels); ir_launch_igemm routes eligible launches to it
bool ir_conv_s1_takes(const IGemmParams& p);
bool ir_conv64_takes(const IGemmParams& p);   // vae_io.hip: 64 -> 64 at full resolution (SwinIR conv_hr)
int ir_launch_conv64(const IGemmParams& p, hipStream_t s, bool force = false);   // force: take the shape whatever IR_CONV64 says (ir_op_conv64)
// "nearest-2x upsample + 3 x 3 conv" as four 2 x 2 convs on the low-resolution tensor (conv_s1.hip); p.up2x2 = 1, p.wgt = the phase matrices
bool ir_conv_s1_up2x2_takes(const IGemmParams& p);
int ir_conv_s1_up2x2_tiles(const IGemmParams& p);
int ir_launch_conv_s1_up2x2(const IGemmParams& p, hipStream_t s);
int ir_conv_s1_tiles(const IGemmParams& p);   // pixel tiles per image (fused GroupNorm statistics: one partial per tile)
int ir_launch_conv_s1(const IGemmParams& p, hipStream_t s);
// conv_s1_fp8.hip: the same structure on e4m3 operands (p.fp8 launches with Cin a multiple of 128 channels)
bool ir_conv_s1_fp8_takes(const IGemmParams& p);
int ir_launch_conv_s1_fp8(const IGemmParams& p, hipStream_t s);

// ---- norms (norm.hip)
static inline int ir_gn_chunks(long HW) {
    long c = HW / 2048;
    if (c < 1) c = 1;
    if (c > 1024) c = 1024;
    return (int)c;
}
// workspace floats needed by ir_launch_groupnorm
static inline long ir_gn_ws_floats(int N, long HW, int C) {
    const long part = (long)N * ir_gn_chunks(HW) * 2 * C, part2 = (long)N * 256 * 64;  // stand-alone partials | fused second stage
    return (part > part2 ? part : part2) + 2L * N * C;
}
// out_fp8 != 0: y receives OCP e4m3 bytes of (result * out_mul) instead of bf16 (the input of an fp8 convolution)
int ir_launch_groupnorm(const bf16_t* x, bf16_t* y, const float* gamma, const float* beta, float* ws, int N, long HW, int C,
                        int G, float eps, int do_silu, hipStream_t s, int out_fp8 = 0, float out_mul = 1.f);
// Same, with the statistics already reduced to per-group partials by the producing conv (IGemmParams::gn_part, `chunks` tiles per
// image): only the finalise and apply launches run. ws needs 2*N*C + N*256*64 floats (scale, shift, second-stage partials).
int ir_launch_groupnorm_fused(const bf16_t* x, bf16_t* y, const float* gamma, const float* beta, const float* part, float* ws, int N,
                              long HW, int C, int G, int chunks, float eps, int do_silu, hipStream_t s, int out_fp8 = 0, float out_mul = 1.f);
// y (bf16, may be null) and yf (fp32, may be null) both receive xn*a + b; columns C..ldy-1 are written as zero.
// DiT self-attention token preparation (norm.hip): KV compression (depthwise r x r / stride r over the token grid + optional LayerNorm) and qk_norm (r = 1)
int ir_launch_dit_token_prep(const bf16_t* in, bf16_t* out, const float* w, const float* bias, const float* gamma, const float* beta, int B, int gh, int gw, int r,
                             int C, int in_rs, long in_bs, int out_rs, long out_bs, hipStream_t s);
int ir_launch_layernorm(const float* x, bf16_t* y, float* yf, const float* a, const float* b, long rows, int C, int ldx, int ldy,
                        float eps, long rows_per_batch, int ab_stride, hipStream_t s);
int ir_launch_gemv_f32(const float* w, const float* x, const float* b, float* out, int N, int K, int act, hipStream_t s);

// ---- attention (attention.hip)
struct AttnParams {
    const bf16_t *q, *k, *vt;  // q/k: [B][T][..] rows with head slices; vt: [B][Hh][DV][Tk_pad]
    bf16_t* o;
    long q_bs, k_bs, o_bs;     // batch strides (elements)
    long vt_bs;                // batch stride of vt (0: one K/V set shared by the whole batch); head stride = DV*Tk_pad
    int q_rs, k_rs, o_rs;      // token strides
    int q_hs, k_hs, o_hs;      // head strides
    int B, Hh, Tq, Tk, Tk_pad, D;
    float scale_log2;          // softmax scale * log2(e)
    const float* key_bias;     // optional additive bias per key [B][kb_bs] (natural-log domain)
    long kb_bs;
    int* ovf_flag;             // optional 4 bytes of device scratch: enables the fixed-reference ping-pong kernel (see attention.hip)
    int ovf_map;               // ints available BEHIND ovf_flag[0] (0: none). With B * Hh * ceil(Tq / 256) of them (round 6) flash_attn_pp2_kernel marks the
                               // 256-query workgroups whose fixed reference was outgrown, and the rescaling kernel behind it recomputes only those
                               // instead of the whole launch (one peaky row among 16384 x 16 used to cost 28 x 1.7 ms per image)
    int kv_groups;             // 0 / 1: K, V^T and key bias of item b sit at b * k_bs / vt_bs / kb_bs. G > 1: at (b % G) * ..., G prompt slots shared round-robin
                               // by the B items (B % G == 0; the DiT cross-attention with one prompt per image, item = tile * n + image)
};
// the K / V^T / key-bias batch index of item b (wave-uniform)
__host__ __device__ inline int ir_attn_kv_item(const AttnParams& p, int b) { return p.kv_groups > 1 ? b % p.kv_groups : b; }
int ir_launch_flash_attn(const AttnParams& p, hipStream_t s);
bool ir_flash_attn_is_pp2(const AttnParams& p);   // ir_launch_flash_attn routes p to flash_attn_pp2_kernel (profiler rows)
// DiT self-attention (D = 72, Tk % 64 == 0, no key bias, ovf_flag set) as one wave per SIMD with two query groups (attn_d512.hip)
int ir_launch_flash_attn_pp2(const AttnParams& p, hipStream_t s);
// DiT cross-attention (D = 72, <= 320 keys, optional additive key bias, ovf_flag set) as a persistent one-wave-per-SIMD kernel with the head's
// K / V^T resident in LDS (attn_d512.hip); ir_launch_flash_attn routes to it and queues the rescaling kernel behind it
bool ir_igemm_up2x2_takes(const IGemmParams& p);   // a phase kernel (conv_halo_s1_kernel<0, 4> or conv_halo_kernel<.., PH>) takes this upsampling conv in its sub-pixel form
bool ir_flash_attn_x72_takes(const AttnParams& p);
int ir_launch_flash_attn_x72(const AttnParams& p, hipStream_t s);
// the rescaling 4-wave kernel alone, as the fallback behind a fixed-reference kernel: returns at once unless *p.ovf_flag is set
int ir_launch_flash_attn_fallback(const AttnParams& p, hipStream_t s);
// DiT self-attention on fp8 (e4m3) MFMA operands (attn_fp8.hip; BASELINE.json configs[4]). p as for ir_launch_flash_attn's self-attention form
// (p.vt: the bf16 V^T buffer, only written / read when the overflow fallback runs); v: the V rows (strides of p.k); tiles: scratch of
// ir_attn_fp8_tile_bytes(B, Hh, Tk) bytes for the quantised K / V^T tile images.
size_t ir_attn_fp8_tile_bytes(int B, int Hh, int Tk);
int ir_launch_flash_attn_fp8(const AttnParams& p, const bf16_t* v, uint8_t* tiles, hipStream_t s);
int ir_launch_flash_attn_d512(const bf16_t* q, const bf16_t* k, const bf16_t* vt, bf16_t* o, int T, int rs, int o_rs, long vt_rs,
                              float scale, hipStream_t s, const int* only_if = nullptr);
// d = 512 without the redundant score product (attn_d512.hip): V^T in 32-key tiles [B][T/32][512][32]; a set *ovf_flag afterwards
// means the result must be recomputed by ir_launch_flash_attn_d512 (which is given the flag as `only_if` and returns at once otherwise)
int ir_launch_transpose_v_tiles(const bf16_t* v, bf16_t* vt, int B, int T, int rs, long v_bs, long vt_bs, hipStream_t s, const int* only_if = nullptr);
int ir_launch_flash_attn_d512_v2(const bf16_t* q, const bf16_t* k, const bf16_t* vt_tiles, bf16_t* o, int B, int T, int rs, int o_rs, long qk_bs,
                                 long vt_bs, long o_bs, float scale, int* ovf_flag, hipStream_t s, const int* only_if = nullptr);   // only_if: run only when *only_if != 0
int ir_launch_flash_attn_d512_v2_rows(const bf16_t* q, const bf16_t* k, const bf16_t* vt_tiles, bf16_t* o, int T, int rows, int rs, int o_rs,
                                      float scale, int* ovf_flag, hipStream_t s);   // a query-row shard (q / o offset by the caller), all T keys
int ir_launch_transpose_v(const bf16_t* v, bf16_t* vt, long v_bs, int v_rs, int v_hs, int B, int Hh, int T, int Tpad, int D,
                          int DV, hipStream_t s, const int* only_if = nullptr);
int ir_launch_swin_attn(const bf16_t* qkv, bf16_t* out, const float* biasT, int B, int H, int W, int heads, int ld, int ldo,
                        int shift, float scale, hipStream_t s);
int ir_launch_softmax_rows(const float* x, bf16_t* y, long rows, int cols, long ldx, long ldy, hipStream_t s);
static inline int ir_attn_dv(int D) { return (D + 31) & ~31; }
// keys per row of a V^T buffer for T keys (AttnParams::Tk_pad): whole 64-key tiles, + 64 so that the row stride is no power of two (channel conflicts)
static inline int ir_attn_tk_pad(int T) { return ((T + 63) & ~63) + 64; }

// ---- fused SwinIR block halves (swin_fused.hip)
// out = x + fc2(gelu(fc1(LayerNorm(x)))) on the fp32 residual stream [T][192] (in place allowed); out2: optional bf16 copy
int ir_launch_swin_mlp(const float* x, float* out, bf16_t* out2, const void* w_tiles, const float* vec, long T, int C, int hid_p, float eps,
                       hipStream_t s, const float* next_g = nullptr, const float* next_b = nullptr, const void* qkv_tiles = nullptr,
                       const float* qkv_b = nullptr, int qkv_n = 0);   // qkv_tiles: out2 = the next block's qkv rows [T][qkv_n] instead of its norm1
// window attention of all heads + output projection + residual in one launch (swin_fused.hip): qkv [tokens][576] bf16, xres / out [tokens][192]
// fp32 (may alias), proj_t = proj weights [192][192] bf16 with columns in accumulator order (weights.pack_swinir)
int ir_launch_swin_attn_proj(const bf16_t* qkv, const float* xres, float* out, const void* proj_t, const float* proj_b, const float* biasT, int B,
                             int H, int W, int shift, float scale, hipStream_t s);

// the whole block behind its qkv projection in one launch (swin_block_kernel): the two above back to back with the post-attention row kept in registers;
// x_in / x_out may alias, out2 as in ir_launch_swin_mlp (bf16 copy of the new rows, or the next block's norm1 rows, or - with qkv_tiles - its qkv rows)
int ir_launch_swin_block(const bf16_t* qkv, const float* x_in, float* x_out, bf16_t* out2, const void* proj_t, const float* proj_b, const float* biasT,
                         int B, int H, int W, int shift, float scale, const void* w_tiles, const float* vec, int C, int hid_p, float eps, hipStream_t s,
                         const float* next_g = nullptr, const float* next_b = nullptr, const void* qkv_tiles = nullptr, const float* qkv_b = nullptr,
                         int qkv_n = 0);

// ---- T5 encoder glue (t5.hip)
int ir_launch_t5_embed(const int* ids, const bf16_t* table, float* x, long rows, int D, int vocab, int* bad, hipStream_t s);
int ir_launch_t5_rmsnorm(const float* x, const float* w, bf16_t* yb, float* yf, long rows, int D, float eps, hipStream_t s);
int ir_launch_t5_attn(const bf16_t* qkv, const float* bias, const float* key_mask, bf16_t* out, int B, int T, int H, int dk, hipStream_t s);
int ir_launch_t5_gated_gelu(const bf16_t* ab, bf16_t* out, long rows, int F, hipStream_t s);

// ---- the cache of encoded captions behind ir_t5_encode_prompts (prompt_cache.hip)
// src fp32 [b][T][D] -> cache slots slot0 .. slot0 + b - 1 (fp16, round to nearest even, or fp32); mask_src [b][T] (null: ones) -> cache_mask
int ir_launch_prompt_cache_store(const float* src, const float* mask_src, void* cache, float* cache_mask, int fp16, int slot0, int b, int T, int D,
                                 hipStream_t s);
// image i of n: embeds_out [i][T][D] / bias_out [i][T] from cache slot slots[i], or from the fixed prompt for a slot outside [0, n_slots)
// (a slot >= n_slots also sets *bad_slot when that is not null)
int ir_launch_prompt_gather(const void* cache, const float* cache_mask, int fp16, int n_slots, const int* slots, const float* fixed_embeds,
                            const float* fixed_mask, float* embeds_out, float* bias_out, int n, int T, int D, int* bad_slot, hipStream_t s);

// ---- PNG encoding of uint8 results (png_encode.hip)
// png_encode.hip: zlib streams of Paeth-filtered rows, one dynamic-Huffman block of literals per chunk of IR_PNG_ROWS rows (in the run mode, where shorter,
// one block of literals and distance-1 matches). IR_PNG_ROWS is a build
// constant (8 .. 64 are sensible; ir_png_bound and the workspace follow it). 8 by measured time at 2048 x 2048: 0.49 ms against 0.72 at 16 and 1.11 at 32
// rows (256 / 128 / 64 workgroups on 256 CUs) for files 0.1 - 0.3 % larger (profiles/png_encoder.txt). hist / codes: [n * chunks][260] dwords, header: [n * chunks][40],
// chunk_bytes: [n * chunks], slots: [n * chunks][slot_cap] bytes, 16-byte aligned.
#ifndef IR_PNG_ROWS
#define IR_PNG_ROWS 8
#endif
#define IR_PNG_HEADER_BITS 1106   // 17 + 19 * 3 + 257 * 4 + 4
int ir_launch_png_encode(const uint8_t* img, int n, int h, long pitch, int vh, int vw, uint8_t* out, size_t out_stride, uint32_t* info,
                         uint32_t* hist, uint32_t* codes, uint32_t* header, uint32_t* chunk_bytes, uint8_t* slots, long slot_cap, hipStream_t s);
// The run mode (ir_png_encode_runs): the buffers above, which hold the literal-only side of every chunk, and next to them run_hist / run_codes:
// [n * chunks][IR_PNG_RUNS_SYMS] dwords (run_codes: 286 codes, the header's bit count, the chunk's choice), run_header: [n * chunks]
// [IR_PNG_RUNS_HEADER_WORDS], flags: [n * chunks][ir_png_runs_flag_words(IR_PNG_ROWS * rowlen)] dwords, one bit per filtered byte that starts a
// run. A chunk beyond IR_PNG_RUNS_MAX_CHUNK bytes has no room for its flags in the LDS: such an image takes ir_launch_png_encode.
#define IR_PNG_RUNS_SYMS 288
#define IR_PNG_RUNS_HEADER_WORDS 48   // 17 + 19 * 3 + 287 * 5 = 1509 bits at most
#define IR_PNG_RUNS_MAX_CHUNK (1 << 18)
static inline size_t ir_png_runs_flag_words(size_t chunk_len) { return (chunk_len + 1 + 31) / 32 + 12; }   // + the end's flag, + the words a lookahead of 258 bits may read
int ir_launch_png_encode_runs(const uint8_t* img, int n, int h, long pitch, int vh, int vw, uint8_t* out, size_t out_stride, uint32_t* info,
                              uint32_t* hist, uint32_t* codes, uint32_t* header, uint32_t* chunk_bytes, uint8_t* slots, long slot_cap,
                              uint32_t* run_hist, uint32_t* run_codes, uint32_t* run_header, uint32_t* flags, long flag_words, hipStream_t s);

// ---- JPEG encoding of uint8 results (jpeg_encode.hip)
// jpeg_encode.hip: the entropy-coded segment of a baseline JPEG (standard Huffman tables, restart intervals of restart_mcus MCUs), libjpeg's bytes.
// IR_JPEG_BLOCK_BITS: the most bits one 8 x 8 block can take, 20 for the DC difference (9-bit code + 11 value bits) and 26 for each of the 63 AC
// coefficients (16-bit code + 10 value bits; a zero costs less than that through ZRL / EOB). ir_jpeg_bound_host: ir_jpeg_bound (0 for arguments
// the encoder refuses). ir_jpeg_layout: the workspace of n images of vh x vw (byte offsets; false where the encoder refuses, also for a bound that
// does not fit info's 32 bits): coef [n][MCUs][blocks per MCU][64] int16, raw / ffs / offsets [n * intervals] dwords, slots [n * intervals][slot_cap]
// bytes. ir_launch_jpeg_encode takes that workspace, 16-byte aligned, and returns -1 with nothing launched for arguments it refuses.
#define IR_JPEG_BLOCK_BITS (20 + 63 * 26)
struct IrJpegLayout {
    size_t intervals, slot_cap, coef, raw, ffs, offsets, slots, total;
};
size_t ir_jpeg_bound_host(int h, int w, int subsampling, int restart_mcus);
bool ir_jpeg_layout(int n, int vh, int vw, int subsampling, int restart_mcus, IrJpegLayout* L);
int ir_launch_jpeg_encode(const uint8_t* img, int n, int h, long pitch, int vh, int vw, int quality, int subsampling, int restart_mcus, uint8_t* out,
                          size_t out_stride, uint32_t* info, void* ws, hipStream_t s);

// ---- JPEG decoding into uint8 images (jpeg_decode.hip); ir_jpeg_file: include/instarevive_hip.h
// ir_jpeg_decode_check: 0, or -1 with *why for a record the kernels do not take. ir_jpeg_decode_workspace: the bytes one file of at most h x w
// pixels (any sampling, any restart interval) and stream_bytes needs at subseq_bits, 0 for sizes outside the contract. ir_launch_jpeg_decode: one
// file's chain of launches; coef: NULL (the workspace's) or where the file's coefficients go; ws: that many bytes, 256-byte aligned.
struct ir_jpeg_file;
int ir_jpeg_decode_check(const ir_jpeg_file* f, const char** why);
size_t ir_jpeg_decode_workspace(int h, int w, uint32_t stream_bytes, int subseq_bits);
long ir_jpeg_decode_blocks(const ir_jpeg_file* f);
int ir_launch_jpeg_decode(const ir_jpeg_file* f, int subseq_bits, uint32_t* info, int16_t* coef, void* ws, hipStream_t s);

// ---- PNG decoding into uint8 images (png_decode.hip); ir_png_file and the workspace's sections: include/instarevive_hip.h
// ir_png_decode_check: 0, or -1 with *why for a record the kernels do not take. ir_png_decode_layout: the byte offsets of the workspace's sections
// for files of at most h x w pixels and stream_bytes at span_bits (false for sizes outside the contract); ir_png_decode_workspace: its total, or 0.
// ir_launch_png_decode: one file's chain of launches; ws: that many bytes, 256-byte aligned.
#define IR_PNG_ADLER_CHUNK 16384
#define IR_PNG_UNFILTER_LANES 1024
struct ir_png_file;
struct IrPngLayout {
    size_t spans, entries, cap, chunks, hdr, cand, e_end, e_next, e_len, e_status, e_off, chain, adler, src, lit, bytes, pix, total;
};
int ir_png_decode_check(const ir_png_file* f, const char** why);
bool ir_png_decode_layout(int h, int w, uint32_t stream_bytes, int span_bits, IrPngLayout* L);
size_t ir_png_decode_workspace(int h, int w, uint32_t stream_bytes, int span_bits);
int ir_launch_png_decode(const ir_png_file* f, int span_bits, uint32_t* info, void* ws, const IrPngLayout& L, hipStream_t s);

// ---- Pillow's 8-bit resampling of uint8 images (resample.hip)
// The plan (ir_resample_plan) is an int32 array: a header of IR_RESAMPLE_HEADER ints - [0] IR_RESAMPLE_MAGIC, [1..4] in_h, in_w, out_h, out_w, [5] the
// filter, [6] ksize_h, [7] ksize_v, [8] / [9] the offsets (in ints, from the plan's start) of the horizontal bounds [out_w][2] and coefficients
// [out_w][ksize_h], [10] / [11] the same of the vertical pass ([out_h] rows), [12] the plan's length in ints - and the tables. A skipped pass
// (equal lengths) has ksize 0 and no tables. inter: [n][in_h][inter_pitch] bytes, inter_pitch a multiple of 4, used when both passes run.
#define IR_RESAMPLE_MAGIC 0x52535038
#define IR_RESAMPLE_HEADER 16
int ir_launch_resample_u8(const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int full_h, int full_w,
                          long out_pitch, const int* plan, uint8_t* inter, long inter_pitch, hipStream_t s);
// rows y0 .. y0 + win_h, columns x0 .. x0 + win_w of that result alone; inter: [n][in_h][inter_pitch], win_w samples per row
int ir_launch_resample_u8_window(const uint8_t* in, int n, int in_h, int in_w, long in_pitch, uint8_t* out, int out_h, int out_w, int y0, int x0, int win_h,
                                 int win_w, int full_h, int full_w, long out_pitch, const int* plan, uint8_t* inter, long inter_pitch, hipStream_t s);

// ---- PSNR-Y / SSIM-Y of uint8 images (metrics.hip)
// One workgroup per IR_METRICS_TH x IR_METRICS_TW tile of the 'valid' SSIM map; part: [n][tiles][2] doubles (the tile's squared-error sum and SSIM
// sum), tab: the three 256-entry luma tables c_k * (double)((float)v / 255.0f) in device memory, out: [n][2] = (mse_y, ssim_y).
#define IR_METRICS_TW 64
#define IR_METRICS_TH 16
int ir_launch_metrics_y(const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, const double* tab,
                        double* part, double* out, hipStream_t s);

// ---- LPIPS v0.1 / alex of uint8 images (lpips.hip)
// ir_lpips_plan: the map sizes of a call and its workspace. Conv outputs oh x ow per stage (pool outputs ph x pw in front of conv2 / conv3), two
// ping-pong NHWC fp32 maps for the 2n images (X: conv1 / conv2 / conv3 / conv5, Y: pool1 / pool2 / conv4) and the distance kernel's partial
// sums [n][chunks] doubles (stage k's are first[k] .. first[k] + count[k] - 1). -1 below 31 x 31 or when a row count leaves an int.
struct IrLpipsPlan {
    int oh[5], ow[5], ph[5], pw[5], first[5], count[5], chunks;
    size_t x_bytes, y_bytes, part_bytes, total;
};
int ir_lpips_plan(int n, int h, int w, IrLpipsPlan* plan);
// tab: [3][256] fp32 scaling table, wgt[k]: [K padded to 32][cout] fp32 with K in (ky, kx, c) order, bias[k] / lin[k]: [cout]; out: [n] doubles
int ir_launch_lpips(const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, const float* tab,
                    const float* const* wgt, const float* const* bias, const float* const* lin, void* ws, double* out, hipStream_t s);

// ---- DISTS of uint8 image pairs (dists.hip)
#define IR_DISTS_CONVS 13
#define IR_DISTS_MAPS 6          // the raw image and the five stage outputs
#define IR_DISTS_CHANNELS 1475   // 3 + 64 + 128 + 256 + 512 + 512
#define IR_DISTS_MIN_EDGE 16
// tab: [3][256] fp32 network input of a byte, x01: [256] fp32 (float)v / 255.0f, w[k]: [K padded to 32][cout] fp32 with K in (ky, kx, c) order,
// b[k]: [cout], alpha / beta: [1475] in map order, wsum: sum(alpha) + sum(beta) in fp64
struct IrDistsModel {
    bool ok = false;
    const float *tab = nullptr, *x01 = nullptr, *w[IR_DISTS_CONVS] = {}, *b[IR_DISTS_CONVS] = {}, *alpha = nullptr, *beta = nullptr;
    double wsum = 0.0;
};
// ir_dists_plan: the map sizes of a call (mh x mw: [0] the image, [k] stage k's output, ceil halves) and its workspace: two ping-pong NHWC fp32
// maps of 64 x h x w floats for each of the 2n images (every later map is smaller), the moment kernel's partial sums of the largest map
// ([n][chunks][C][5] doubles, chunks[k] = the 1024-pixel chunks of map k) and the folded moments [n][1475][5] doubles. -1 below 16 x 16 or when a
// row count leaves an int.
struct IrDistsPlan {
    int mh[IR_DISTS_MAPS], mw[IR_DISTS_MAPS], chunks[IR_DISTS_MAPS];
    size_t map_bytes, part_bytes, mom_bytes, total;
};
int ir_dists_plan(int n, int h, int w, IrDistsPlan* plan);
// out: [n] doubles; moments: [n][1475][5] doubles (mx, my, vx, vy, cxy) or null (they then stay in the workspace)
int ir_launch_dists(const IrDistsModel& m, const uint8_t* a, int a_rows, long a_pitch, const uint8_t* b, int b_rows, long b_pitch, int n, int h, int w, void* ws,
                    double* out, double* moments, hipStream_t s);

// ---- FID's Inception-v3 features of uint8 images (fid.hip)
#define IR_FID_SIZE 299
#define IR_FID_DIM 2048
#define IR_FID_CONVS 94
#define IR_FID_BLOCKS 13               // the maps of block_means: Conv2d_2b, Conv2d_4a and the eleven Mixed_* blocks
#define IR_FID_BLOCK_CHANNELS 10304    // 64 + 192 + 256 + 288 + 288 + 5 x 768 + 1280 + 2048 + 2048
#define IR_FID_MIN_EDGE 2
#define IR_FID_MAX_N 4096
#define IR_FID_MAP_FLOATS 1382976      // the largest map of an image: Conv2d_2b's 147 x 147 x 64
// a convolution of the network, in the order the launches take them (and ir_fid_configure binds them); name: torchvision's
struct IrFidConv {
    char name[40];
    int cin, cout, kh, kw, stride, ph, pw;
};
const IrFidConv* ir_fid_convs();   // [IR_FID_CONVS]
// w[k]: [kh kw cin (cin 3 -> 4) padded to 32][cout padded to 64] fp32 with K in (ky, kx, c) order, scale / shift[k]: [cout] the BatchNorm folded in
// fp64 and rounded once; x01: [256] (float)v / 255.0f
struct IrFidModel {
    bool ok = false;
    const float *w[IR_FID_CONVS] = {}, *scale[IR_FID_CONVS] = {}, *shift[IR_FID_CONVS] = {}, *x01 = nullptr;
};
// the workspace of n images: the four-channel input map and four maps of IR_FID_MAP_FLOATS floats per image (two for the trunk, two for the
// branches); it does not depend on the images' size. -1 for n outside 1 .. IR_FID_MAX_N.
struct IrFidPlan {
    size_t x4_bytes, map_bytes, total;
};
int ir_fid_plan(int n, IrFidPlan* plan);
// byte offsets of the parts of ir_fid_resize_plan's tables for h x w images: bounds int[299][2] per axis, coefficients double[299][kx | ky]
struct IrFidTables {
    size_t xb, yb, xk, yk, total;
    int kx, ky;
};
int ir_fid_tables_layout(int h, int w, int mode, IrFidTables* t);   // host (api_image.cpp); mode: IR_FID_RESIZE_*; -1 for a bad size or mode
// features: [n][2048] doubles; block_means: [n][10304] doubles or null; resized: [n][299][299][3] floats or null
int ir_launch_fid(const IrFidModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, int mode, const void* tables, double* features,
                  double* block_means, float* resized, void* ws, hipStream_t s);

// ---- NIQE's block statistics of uint8 images (niqe.hip)
// One workgroup per IR_NIQE_BLOCK x IR_NIQE_BLOCK block of the top-left (h / 96 * 96) x (w / 96 * 96) rectangle. tab: four 256-entry fp64 tables in
// device memory - coef_c * (double)((float)v / 255.0f) for 0.299 / 0.587 / 0.114, then v / 255.0; half: [n][H / 2][W / 2] doubles (the half-size
// luma plane); out: [n][2][blocks][5][6] doubles. ir_niqe_window_host: the 7 x 7 window the kernels use.
#define IR_NIQE_BLOCK 96
void ir_niqe_window_host(double* k49);
int ir_launch_niqe_stats(const uint8_t* img, int rows, long pitch, int n, int h, int w, const double* tab, double* half, double* out, hipStream_t s);

// ---- IL-NIQE's dense fp64 2-D DFT and Weibull fit (ilniqe.hip)
// ir_ilniqe_twiddles_host: cos and sin of 2 pi (jk mod N) / N as [N][N] doubles each. ir_launch_dft2_f64: the 2-D DFT of an N x N plane (N = 252 or
// 504; im may be null for a real input), forward (exp(-i ..), unscaled) or inverse (exp(+i ..), times 1 / N^2), as two complex matrix products on
// the fp64 MFMA; tw_cos / tw_sin: the device copies of the twiddles of that N; ws: 2 N N doubles. The outputs must not overlap the inputs.
// ir_launch_weibull_fit: (k, lambda) of each of `rows` rows of `count` positive doubles (2 .. IR_WEIBULL_MAX), out [rows][2].
#define IR_WEIBULL_MAX 7056
void ir_ilniqe_twiddles_host(int N, double* cos_nn, double* sin_nn);
int ir_launch_dft2_f64(const double* tw_cos, const double* tw_sin, const double* re, const double* im, int N, int inverse, double* out_re, double* out_im,
                       double* ws, hipStream_t s);
int ir_launch_weibull_fit(const double* x, int rows, int count, double* k_lambda, hipStream_t s);
// ir_ilniqe_stats. IrIlniqeTables: the device tables ir_ilniqe_configure binds - tw[0], tw[1]: cos | sin of 252 and 504; bank[0], bank[1]: the twelve
// log-Gabor filters [12][N][N] of 252 and 504; host copies of the 5 x 5 and 6 x 6 windows and of the derivative taps [scale][x g | g][11].
// ir_ilniqe_plan_host fills the resize tables of one input size (ir_ilniqe_plan_layout bytes: idx0 [524][P0] and idx1 [524][P1] as int, padded to
// 8 bytes, then w0 and w1 as doubles; P = ir_ilniqe_taps(n_in)). out: [n][2][36][IR_ILNIQE_STATS] doubles per scale and block: 5 x 6 AGGD
// numbers of plane 0's fields, 78 x 6 of planes 7-84, 3 x (mean, variance) of planes 4-6, 27 x (k, lambda) of planes 1-3 and 85-108.
#define IR_ILNIQE_SIZE 524
#define IR_ILNIQE_USED 504
#define IR_ILNIQE_BLOCK 84
#define IR_ILNIQE_STATS 558
struct IrIlniqeTables {
    bool ok = false;
    const double* tw[2] = {nullptr, nullptr};
    const double* bank[2] = {nullptr, nullptr};
    double win5[25], win6[36], taps[2][22];
};
int ir_ilniqe_taps(int n_in);
size_t ir_ilniqe_plan_layout(int h, int w, size_t* idx1, size_t* w0, size_t* w1);
void ir_ilniqe_plan_host(int h, int w, void* tables);
size_t ir_ilniqe_workspace(int w);
int ir_launch_ilniqe_stats(const IrIlniqeTables& tb, const uint8_t* img, int rows, long pitch, int n, int h, int w, const void* plan, double* out,
                           double* ws, hipStream_t s);

// ---- CLIP-IQA of uint8 images (clipiqa.hip)
// The bound model: every convolution as w [K padded to 32][cout] fp32 with K in (ky, kx, c) order and the folded BatchNorm as scale / shift [cout];
// the stem's three, then the bottleneck blocks in order (down: the identity branch's 1 x 1, present when the stride is 2 or the counts differ);
// the attention pool's four linears as PyTorch holds them ([out][in] fp32, bias [out]); text: [2 * n_pairs][out_dim] fp32 unit rows.
struct IrClipConv {
    int cin = 0, cout = 0, ks = 0;
    const float *w = nullptr, *scale = nullptr, *shift = nullptr;
};
struct IrClipBlock {
    IrClipConv c1, c2, c3, down;
    int stride = 1;
    bool has_down = false;
};
#define IR_CLIPIQA_MAX_BLOCKS 64
struct IrClipiqaModel {
    bool ok = false;
    int layers[4] = {}, width = 0, heads = 0, out_dim = 0, n_pairs = 0, n_blocks = 0;
    double logit_scale = 0.0;
    const float* tab = nullptr;   // [3][256] input table
    IrClipConv stem[3];
    IrClipBlock blocks[IR_CLIPIQA_MAX_BLOCKS];
    const float *qw = nullptr, *qb = nullptr, *kw = nullptr, *kb = nullptr, *vw = nullptr, *vb = nullptr, *cw = nullptr, *cb = nullptr, *text = nullptr;
};
// ir_clipiqa_plan: the workspace of a call - five NHWC fp32 map slots for the n images (0 / 1: a block's input and output in turn, 2: conv1's
// output, the pooled conv2 output and the pooled identity input, 3: conv2's output, 4: the identity branch) and the fp64 tail's eight arrays
// (token mean, q, u, c0, the [T][heads] probabilities, y, the attention output, the feature). Byte offsets; fh x fw is the last map.
// -1 below 32 x 32, for more than 65535 images or when a row count leaves an int.
struct IrClipiqaPlan {
    size_t slot[5], tail[8], total;
    int fh, fw, final_slot;
};
int ir_clipiqa_plan(const IrClipiqaModel& m, int n, int h, int w, IrClipiqaPlan* plan);
int ir_launch_clipiqa(const IrClipiqaModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws,
                      hipStream_t s);

// ---- MUSIQ of uint8 images (musiq.hip)
// ir_musiq_layout_host (host only): the scales of an h x w image - scale s is the image resized so that its longer side is longer[s], or the image
// itself where longer[s] is 0 - with their 'SAME' patch grids, the first patch of each scale in the image's patch list, and the factors
// (float)grid / count of the hashed spatial index. -1 when a resized side rounds to 0 or the token count leaves an int.
#define IR_MUSIQ_MAX_SCALES 4
#define IR_MUSIQ_MAX_LAYERS 64
struct IrMusiqScale {
    int rh, rw, count_h, count_w, pad_top, pad_left, first, resized;
    float fh, fw;
};
struct IrMusiqLayout {
    int n_scales, patches, T;   // T = 1 + patches
    IrMusiqScale s[IR_MUSIQ_MAX_SCALES];
};
int ir_musiq_layout_host(int h, int w, int patch, int grid, int n_scales, const int* longer, IrMusiqLayout* lay);
void ir_musiq_input_table_host(float* tab256);
// The bound model: the standardised conv weights as [K padded to 32][cout] with K in (ky, kx, c) order, every linear as [in][out] (q | k | v side by
// side), the GroupNorm / LayerNorm vectors and the embeddings as they were uploaded.
struct IrMusiqBlock {
    const float *ln1g, *ln1b, *qkvw, *qkvb, *ow, *ob, *ln2g, *ln2b, *f1w, *f1b, *f2w, *f2b;
};
struct IrMusiqModel {
    bool ok = false;
    int patch = 0, hidden = 0, mlp = 0, heads = 0, layers = 0, grid = 0, n_scales = 0, longer[IR_MUSIQ_MAX_SCALES] = {};
    const float* tab = nullptr;   // [256] input table
    const float *stem_w = nullptr, *stem_g = nullptr, *stem_b = nullptr;
    const float *cw[4] = {}, *cg[4] = {}, *cb[4] = {};   // the bottleneck's conv1, conv2, conv3 and its projection branch
    const float *emb_w = nullptr, *emb_b = nullptr, *pos = nullptr, *semb = nullptr, *cls = nullptr;
    const float *fin_g = nullptr, *fin_b = nullptr, *head_w = nullptr, *head_b = nullptr;
    IrMusiqBlock blk[IR_MUSIQ_MAX_LAYERS] = {};
};
// ir_musiq_plan: the workspace of a call, byte offsets. Per patch of the n images: two slots of 16384 floats (A: the stem conv's map, later the
// bottleneck's output; B: the patch's input pixels, later the projection branch) and three of 4096 (the pooled map, conv1's and conv2's output);
// behind them the patch embeddings. The transformer's arrays (x, the LayerNorm output, q | k | v, the attention output, the MLP's hidden rows and
// the scores of zc (image, head) pairs at a time, rows padded to Tpad) lie over the patch slots, which are dead by then.
struct IrMusiqPlan {
    IrMusiqLayout lay;
    size_t slot[5], emb, x, hn, qkv, o, f, s, total;
    int zc, Tpad;
};
int ir_musiq_plan(const IrMusiqModel& m, int n, int h, int w, IrMusiqPlan* plan);
int ir_launch_musiq(const IrMusiqModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, void* ws,
                    hipStream_t s);

// ---- MANIQA of uint8 images (maniqa.hip)
#define IR_MANIQA_MAX_LAYERS 32
#define IR_MANIQA_MAX_DEPTH 4
#define IR_MANIQA_SWIN_LAYERS 2
#define IR_MANIQA_MAX_CROPS 1024
void ir_maniqa_input_table_host(float* tab256);
// host only: the uniform grid of crop origins (y, x) - step (side - crop) / floor(sqrt(crops)) per axis, ceil(sqrt(crops)) positions per axis, y
// outer, the first `crops` of them. -1 for min(h, w) <= crop, crops outside 1 .. IR_MANIQA_MAX_CROPS.
int ir_maniqa_crops_host(int h, int w, int crop, int crops, int* out_yx);
// The bound model: every linear as [in][out] (q | k | v as they are stored, side by side), the patch conv as [(c, ky, kx)][embed], the norm
// vectors, embeddings and relative-position tables as they were uploaded. A block of the ViT has no rpb.
struct IrManiqaBlock {
    const float *ln1g, *ln1b, *qkvw, *qkvb, *pw, *pb, *ln2g, *ln2b, *f1w, *f1b, *f2w, *f2b, *rpb;
};
struct IrManiqaModel {
    bool ok = false;
    int crop = 0, patch = 0, embed = 0, vit_heads = 0, vit_mlp = 0, vit_layers = 0, taps[4] = {}, window = 0, swin_heads = 0, swin_depth = 0, dim_mlp = 0;
    float scale = 0.f;
    const float* tab = nullptr;   // [256] input table
    const float *patch_w = nullptr, *patch_b = nullptr, *cls = nullptr, *pos = nullptr;
    IrManiqaBlock vit[IR_MANIQA_MAX_LAYERS] = {};
    const float *tabw[2][2] = {}, *tabb[2][2] = {};   // [stage][k]: [N][3 N] and [3 N]
    const float *convw[2] = {}, *convb[2] = {};       // [in][out]
    IrManiqaBlock swin[2][IR_MANIQA_SWIN_LAYERS][IR_MANIQA_MAX_DEPTH] = {};
    const float *head_w1 = nullptr, *head_b1 = nullptr, *head_w2 = nullptr, *head_b2 = nullptr;   // fc1 of score | weight [Eh][2 Eh], [2 Eh]; fc2 [2][Eh], [2]
};
// ir_maniqa_plan: the workspace of a call that processes its n * crops crops in passes of per_pass (cut to n * crops), byte offsets. In front the
// per-patch (s, w) doubles of ALL crops and the two maps [4 embed][N] per crop of a pass that the TABs alternate between; behind them, over one
// another, the trunk's arrays (x, the LayerNorm output, q | k | v, the attention output, the MLP's hidden rows, the scores of zc (crop, head)
// pairs with rows padded to Tpad, the patch embeddings), a TAB's (q | k | v of every crop, one crop's C x C matrix) and a Swin stage's.
struct IrManiqaPlan {
    size_t sw, tap[2], x, hn, qkv, o, f, s, emb, tqkv, ts, y0, y, yn, sqkv, so, sf, total;
    int cp, zc, Tpad;
};
int ir_maniqa_plan(const IrManiqaModel& m, int n, int crops, int per_pass, IrManiqaPlan* plan);
int ir_launch_maniqa(const IrManiqaModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, const int* origins, int crops, double* scores,
                     float* feat, void* ws, const IrManiqaPlan& plan, hipStream_t s);

// ---- TOPIQ-NR of uint8 images (topiq.hip)
#define IR_TOPIQ_MAX_BLOCKS 64
#define IR_TOPIQ_GATE_HIDDEN 64
#define IR_TOPIQ_EMB 32
#define IR_TOPIQ_MIN_EDGE 16
#define IR_TOPIQ_MAX_DIM 2048
void ir_topiq_input_table_host(float* tab768);
// The bound model: every conv as [K padded to 32][cout] with K in (ky, kx, c) order and its folded BatchNorm (scale null: shift is the bias), every
// linear and 1 x 1 conv of the head as [in][out] (q | k | v side by side as in_proj packs them), the gate's last conv as [(ky, kx, c)], the
// score head's linears as they were uploaded ([out][in]: the fp64 tail reads rows).
struct IrTopiqConv {
    const float *w = nullptr, *scale = nullptr, *shift = nullptr;
    int cin = 0, cout = 0, ks = 0, stride = 1;
};
struct IrTopiqBlock {
    IrTopiqConv c1, c2, c3, down;
    int has_down = 0;
};
struct IrTopiqAttn {
    const float *n1g, *n1b, *n2g, *n2b, *n3g, *n3b, *inw, *inb, *ow, *ob, *f1w, *f1b, *f2w, *f2b;
};
struct IrTopiqGate {
    const float *sw, *sb, *w1, *b1, *w3, *b3, *rw, *rb;   // splitconv [C][2 C], the gate's 1 x 1 [C][64], its last conv [576], dim_reduce [C][D]
    IrTopiqConv c2;                                        // the gate's 3 x 3, 64 -> 64
};
struct IrTopiqModel {
    bool ok = false;
    int depths[4] = {}, width = 0, dim = 0, heads = 0, ffn = 0, n_blocks = 0;
    const float* tab = nullptr;   // [3][256] input table
    IrTopiqConv stem;
    IrTopiqBlock blocks[IR_TOPIQ_MAX_BLOCKS];
    IrTopiqGate gate[5] = {};
    IrTopiqAttn sa[5] = {}, ca[4] = {}, pool = {};
    const float *h_emb = nullptr, *w_emb = nullptr;
    const float* sc[10] = {};   // score.0.{weight,bias}, score.1.*, score.3.*, score.4.*, score.6.*
};
// ir_topiq_plan: the workspace of a call, byte offsets - the trunk's five NHWC map slots as ir_clipiqa_plan has them, the gate's maps (x2, then x1
// over it; the two hidden maps), the pooled map, the tokens of the five levels, and the transformer's arrays (two LayerNorm outputs, q | k | v,
// the attention output, the FFN's hidden rows, the score matrices of as many (image, head) pairs as one launch takes). H x W: the feature maps,
// TH x TW: the token grids. -1 below 16 x 16, for more than 65535 images or when a row count leaves an int.
struct IrTopiqPlan {
    int H[5], W[5], TH[5], TW[5];
    size_t slot[5], ga, gh1, gh2, pooled, tok[5], hn, hm, qkv, o, f, s, total;
};
int ir_topiq_plan(const IrTopiqModel& m, int n, int h, int w, IrTopiqPlan* plan);
int ir_launch_topiq(const IrTopiqModel& m, const uint8_t* img, int rows, long pitch, int n, int h, int w, double* scores, float* feat, float* level_means,
                    void* ws, hipStream_t s);

// ---- low-quality inputs from ground truth (degrade.hip)
// One image: blur (K x K fp64 taps in device memory, K odd, at most IR_DEGRADE_MAX_KSIZE: the float halo tile of a 32 x 32 patch must fit in 64 KB
// of LDS), bilinear to lh x lw, noise (or NULL), the JPEG round trip at q (0: none), bilinear back, bytes (norm: include/instarevive_hip.h's IR_DEGRADE_NORM_*). jpeg: NULL or lh x lw x 3 bytes behind
// the JPEG step (written when q > 0). ws: ir_degrade_workspace(h, w) bytes, 256-byte aligned. Returns -1 with nothing launched for a size the
// kernels do not take. ir_degrade_qtables_host: jpeg_set_quality's two tables (natural order) for q in 1 .. 100.
#define IR_DEGRADE_MAX_KSIZE 41
#define IR_DEGRADE_MIN_LOW 8
void ir_degrade_qtables_host(int q, uint16_t* luma64, uint16_t* chroma64);
size_t ir_degrade_workspace(int h, int w);
int ir_launch_degrade(const uint8_t* img, long pitch, int h, int w, const double* k, int K, int lh, int lw, float sigma, int q, const float* noise,
                      int norm, uint8_t* out, long out_pitch, uint8_t* jpeg, void* ws, hipStream_t s);

// ---- the second-order degradation chain (degrade_chain.hip); ir_chain: include/instarevive_hip.h
// check: walks one image's ops (host) -> 0 and the largest height and width among its images, or -1 and the reason. workspace: two float images of the
// largest size, the DiffJPEG planes and the presence array. launch: the chain of one image, ws 256-byte aligned; the chain has passed check.
#define IR_CHAIN_MAX_KSIZE 21
#define IR_CHAIN_MAX_SIDE 8192
struct ir_chain;
int ir_degrade_chain_check(const ir_chain* ch, int h, int w, int* max_ih, int* max_iw, const char** why);
size_t ir_degrade_chain_workspace(int h, int w, int max_ih, int max_iw);
int ir_launch_degrade_chain(const uint8_t* img, long pitch, int h, int w, const ir_chain* ch, int max_ih, int max_iw, uint8_t* out, long out_pitch,
                            float* tap, void* ws, hipStream_t s);

// ---- layout / elementwise (elementwise.hip)
int ir_launch_u8_to_nchw(const uint8_t* in, float* out, int N, int H, int W, hipStream_t s);
int ir_launch_swin_prep(const float* x_nchw, bf16_t* out, int N, int H, int W, const float* mean3, float img_range, hipStream_t s);
int ir_launch_nhwc_to_nchw(const float* in, int in_cs, float* out, int N, int C, long HW, float scale, float shift, int clamp01,
                           hipStream_t s);
int ir_launch_nchw_to_nhwc_bf16(const float* in, bf16_t* out, int N, int C, long HW, int Cpad, float scale, float shift,
                                hipStream_t s);
int ir_launch_nhwc_f32_to_bf16pad(const float* in, int in_cs, bf16_t* out, long npix, int C, int Cpad, float scale, float shift,
                                  hipStream_t s);
int ir_launch_quant_mean(const float* h8, int h_cs, const float* wq, const float* bq, float* lat_nchw, int N, long HW, float scale,
                         hipStream_t s);
int ir_launch_latent_prep(const float* lat_nchw, const float* wpq, const float* bpq, bf16_t* out, int N, long HW, int Cpad,
                          float in_scale, hipStream_t s);
int ir_launch_patchify(const float* lat_nchw, bf16_t* out, int N, int h, int w, int Cpad, hipStream_t s);
int ir_launch_unpatchify(const float* tok, float* out_nchw, int N, int h, int w, hipStream_t s);
int ir_launch_eps_to_x0(const float* tok, const float* lat_in, float* lat_out, int N, int h, int w, float sqrt_acp,
                        float sqrt_1macp, float out_scale, hipStream_t s);
int ir_launch_nhwc_to_u8(const float* in, int in_cs, uint8_t* out, long npix, float scale, float shift, hipStream_t s);
int ir_launch_nchw_to_u8(const float* in, uint8_t* out, int N, long HW, hipStream_t s);
int ir_launch_zero_f32(float* p, long n, hipStream_t s);
// vae_io.hip: the VAE's first / last convolution at full resolution as HBM-bound kernels of their own
int ir_vae_conv_in_tiles(int H, int W);   // GroupNorm partial tiles per image ir_launch_vae_conv_in writes (the gn_chunks of the following GroupNorm)
int ir_launch_vae_conv_in(const float* in, const bf16_t* wgt, const float* bias, bf16_t* out, float* gn_part, int N, int H, int W, float in_scale,
                          float in_shift, hipStream_t s);
int ir_launch_vae_norm_conv_out(const bf16_t* x, const float* scale, const float* shift, const bf16_t* wgt, const float* bias, float* out, int N, int H,
                                int W, hipStream_t s);
int ir_launch_conv64_to3(const bf16_t* x, const bf16_t* wgt, const float* bias, float* out, int N, int H, int W, hipStream_t s);   // SwinIR conv_last (64 -> 3), same kernel family
int ir_launch_fill_u32(uint32_t* p, long n, uint32_t v, hipStream_t s);
int ir_launch_count_flag(const int* flag, int* counter, hipStream_t s);   // *counter += 1 if *flag != 0 (diagnostic: ir_attn_fallback_count)
int ir_launch_tile_add(float* dst, const float* src, int N, int C, int H, int W, int th, int tw, int y0, int x0, hipStream_t s);
int ir_launch_tile_div(float* dst, int N, int C, int H, int W, int th, int tw, int sy, int sx, hipStream_t s);
int ir_launch_crop_nchw(const float* src, float* dst, int N, int C, int H, int W, int y0, int x0, int th, int tw, float scale,
                        hipStream_t s);
int ir_launch_wavelet_fix(const float* content, const float* style, float* out, float* tmp, int N, int H, int W, hipStream_t s);
int ir_launch_adain_fix(const float* content, const float* style, float* out, float* ws, int N, int H, int W, hipStream_t s);
int ir_launch_silu_f32(const float* in, float* out, long n, hipStream_t s);
int ir_launch_timestep_embed(float* out, float t, int dim, hipStream_t s);
int ir_launch_f32_to_bf16(const float* in, bf16_t* out, long n, hipStream_t s);
int ir_launch_modtab(const float* t, const float* sst, float* out, int L, int R, int C, int t_stride, int scale_mask, hipStream_t s);
int ir_launch_add_bias_rows(float* x, const float* b, long n, int C, hipStream_t s);

// attn_d512_fp8.hip: the VAE mid-block attention (d = 512) on fp8 (e4m3) MFMA operands (BASELINE.json configs[4]); T % 128 == 0, T >= 256
size_t ir_attn_d512_fp8_tile_bytes(int B, int T);
bool ir_attn_d512_fp8_takes(int T);
int ir_launch_flash_attn_d512_fp8(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* o, uint8_t* tiles, int B, int T, int rs, int o_rs,
                                  long qk_bs, long o_bs, float scale, int* ovf_flag, hipStream_t s);

// unet.hip: memory-bound kernels of the ControlLDM path (GroupNorm over any channel count, GEGLU, latent ends, skip rows)
int ir_gn_any_chunks(long HW);
long ir_gn_any_ws_floats(int N, long HW, int C);
int ir_launch_groupnorm_any(const bf16_t* x, bf16_t* y, const float* gamma, const float* beta, float* ws, int N, long HW, int C, int G, float eps,
                            int do_silu, hipStream_t s);
int ir_launch_geglu(const bf16_t* ag, bf16_t* out, long rows, int F, hipStream_t s);
int ir_launch_cldm_in(const float* x, const float* hint, bf16_t* out, int N, long HW, hipStream_t s);
int ir_launch_cldm_out(const float* zT, const float* v, int v_cs, float* out, int N, long HW, hipStream_t s);
int ir_launch_copy_rows(const bf16_t* src, int src_cs, const bf16_t* add, int add_cs, bf16_t* dst, int dst_cs, long rows, int C, hipStream_t s);
