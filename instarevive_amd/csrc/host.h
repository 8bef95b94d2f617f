// What the host translation units of the C-ABI layer share: the context, the weight and model structs it contains, and the few helpers every
// entry point uses. api.cpp holds the models and their stages, api_image.cpp the image tools. Private to csrc/; the contract is
// include/instarevive_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/instarevive_hip.h"
#include "kernels.h"

// A named namespace: ir_ctx contains these types, so they have to be the same types in every file that includes this header.
namespace ir_host {

struct Tensor {
    void* p = nullptr;
    size_t bytes = 0;
};

struct Conv {  // packed conv / linear weight: w [cout_pad][taps*cin] bf16, b [cout_pad] fp32
    const bf16_t* w = nullptr;
    const float* b = nullptr;
    int cin = 0, cout = 0, cout_pad = 0, taps = 1;
    int cin_r = 0, cout_r = 0;  // un-padded channel counts for the algorithmic FLOP count of the profiler (0: cin / cout)
    long w_rs = 0;  // weight row stride in elements (0: taps*cin, densely packed)
    // optional fp8 form (BASELINE.json configs[4]): OCP e4m3 weights [cout][9][cin] quantised per output channel, the dequantisation
    // factor per channel (weight scale / activation scale) and the bias divided by it (see IGemmParams::fp8)
    const uint8_t* w8 = nullptr;
    const float *g8 = nullptr, *b8 = nullptr;
    // optional sub-pixel phase matrices of a conv that follows a nearest-2x upsample: [4][cout][4][cin] bf16 (weights.pack_conv_up2x2)
    const bf16_t* wup = nullptr;
};
struct Norm {
    const float *g = nullptr, *b = nullptr;
    int c = 0;
};

struct SwinBlock {
    Norm n1, n2;
    Conv qkv, proj, fc1, fc2;
    const float* biasT = nullptr;
    const float* biasM = nullptr;  // shifted blocks: [4 window classes][heads][64][64] bias tables with the attention mask folded in (the fused kernels), optional
    const void* mlp_t = nullptr;   // weight tiles + vectors of the fused LN2 -> fc1 -> GELU -> fc2 -> + x kernel (swin_fused.hip), optional
    const float* mlp_v = nullptr;
    const void* proj_t = nullptr;  // proj weights with columns in accumulator order for the fused window attention + projection kernel, optional
    const void* qkv_t = nullptr;   // qkv weights as ring tiles of swin_mlp_kernel: the PREVIOUS block's fused MLP launch also makes this block's qkv rows, optional
};
struct SwinLayer {
    std::vector<SwinBlock> blocks;
    Conv conv;
};
struct SwinModel {
    bool ok = false;
    int C = 0, Cp = 0, heads = 0, hid = 0, hid_p = 0, nf = 0;
    float range = 1.f, mean[3] = {0, 0, 0};
    Conv conv_first, after_body, before_up, up1, up2, up3, hr, last;
    Norm pe, norm;
    std::vector<SwinLayer> layers;
};

struct ResW {
    Norm n1, n2;
    Conv c1, c2, sc;
    bool has_sc = false;
};
struct AttnW {
    Norm n;
    Conv q, k, v, o;
};
struct VaeLevel {
    std::vector<ResW> res;
    bool has_resample = false;
    Conv resample;
};
struct VaeHalf {
    bool ok = false;
    Conv conv_in, conv_out;
    std::vector<VaeLevel> levels;  // index = i_level (ldm numbering)
    ResW mid1, mid2;
    AttnW attn;
    Norm norm_out;
    int cmax = 0;
};
struct VaeModel {
    VaeHalf enc, dec;
    const float *qw = nullptr, *qb = nullptr, *pqw = nullptr, *pqb = nullptr;
};

struct DitLayer {
    const float* sst = nullptr;
    Conv qkv, ao, cq, ckv, co, fc1, fc2;
    bf16_t* kc = nullptr;   // [P][n_tok][2*hidden] cached K|V of the prompts (P = DitModel::n_prompts; rows for prompt_slots x tok_pad allocated)
    bf16_t* vtc = nullptr;  // [P][heads][DV][tok_pad]
    // optional branches of the self-attention (AttentionKVCompress, PixArt_blocks.py:60-158; round 6): KV token compression by a depthwise r x r / stride r
    // convolution over the token grid (kvc_w [C][r*r], kvc_b; 'uniform' / 'ave' sampling arrive as a weight of 1 on the first tap) with an optional LayerNorm
    // (kvc_g / kvc_beta: the 'conv' sampler's `norm`), and LayerNorm on q and k (qk_norm)
    int kvc_r = 1;
    const float *kvc_w = nullptr, *kvc_b = nullptr, *kvc_g = nullptr, *kvc_beta = nullptr, *qn_g = nullptr, *qn_b = nullptr, *kn_g = nullptr, *kn_b = nullptr;
};
struct DitModel {
    bool ok = false, prompt_ok = false;
    int L = 0, heads = 0, hd = 0, C = 0, mlp = 0, cap = 0, base = 0;
    Conv patch, cap1, cap2, fin;
    const float *t1w = nullptr, *t1b = nullptr, *t2w = nullptr, *t2b = nullptr, *tbw = nullptr, *tbb = nullptr, *fsst = nullptr;
    std::vector<DitLayer> layers;
    // ControlNet-Half branch (transformer_controlnet.py:58-76): copies of the first ncopy blocks, each followed by after_proj;
    // before_proj in front of copy 0. Empty unless ir_dit_control_configure ran.
    int ncopy = 0;
    std::vector<DitLayer> ctrl;
    std::vector<Conv> after;
    Conv before;
    int n_tok = 0, tok_pad = 0;
    float* key_bias = nullptr;   // [P][n_tok]
    // prompt slots (ir_dit_set_prompts): item b of every cross-attention launch attends to slot b % n_prompts; the slot strides of kc / vtc /
    // key_bias (elements) are 0 while one prompt is set, so that launch is today's single-prompt one
    int n_prompts = 1;
    long kc_slot = 0, vt_slot = 0, kb_slot = 0;
    // timestep-dependent tables (recomputed when the timestep changes)
    float cached_t = -1e30f;
    float *tsin = nullptr, *th = nullptr, *emb = nullptr, *semb = nullptr, *t6 = nullptr, *modtab = nullptr, *fmod = nullptr;
    float* ctrl_modtab = nullptr;
    // Micro-conditioning (round 6; scripts/DMD/transformer_train/generate.py:56-62 builds `resolution` / `aspect_ratio` when config.sample_size == 128;
    // diffusers' PixArtAlphaCombinedTimestepSizeEmbeddings, whose in-tree twin is SizeEmbedder, PixArt_blocks.py:366-399, wired as in
    // diffusion/model/nets/controlnet.py:189-191): S = C / 3 > 0 when the host uploaded the two embedders (dit.res1 / dit.res2 / dit.ar1 / dit.ar2). The
    // conditioning vector is then emb(t) + [size_emb(h) | size_emb(w) | ar_emb(h / w)] of the LATENT's height and width, so the tables also depend on them.
    int S = 0;
    const float *rs1w = nullptr, *rs1b = nullptr, *rs2w = nullptr, *ar1w = nullptr, *ar1b = nullptr, *ar2w = nullptr;
    float *tsin2 = nullptr, *th2 = nullptr;
    int cached_h = -1, cached_w = -1;
};

// T5 v1.1 encoder (prompt producer, diffusion/model/t5.py:82-101)
struct T5Layer {
    const float *ln1 = nullptr, *ln2 = nullptr;
    Conv qkv, o, wi, wo;   // q|k|v fused [3*H*dk][D]; wi_0|wi_1 fused [2F][D]
};
struct T5Model {
    bool ok = false;
    int L = 0, D = 0, H = 0, dk = 0, F = 0, vocab = 0;
    const bf16_t* embed = nullptr;
    const float* final_ln = nullptr;
    std::vector<T5Layer> layers;
    int* bad = nullptr;   // device flag: an input id was outside the vocabulary
};


// OpenCLIP text tower of the ControlLDM path's cond_stage_model (FrozenOpenCLIPEmbedder.encode_with_transformer, ldm/modules/encoders/modules.py:
// 176-193: token + positional embedding, pre-LN transformer blocks with a causal mask, ln_final)
struct ClipLayer {
    Norm n1, n2;
    Conv qkv, o, fc, proj;   // in_proj (q rows pre-scaled by d_head^-0.5), out_proj, mlp.c_fc, mlp.c_proj
};
struct ClipTextModel {
    bool ok = false;
    int L = 0, D = 0, H = 0, dk = 0, F = 0, vocab = 0, T = 0;
    const bf16_t* embed = nullptr;
    const float *pos = nullptr, *causal = nullptr;   // [T][D]; [H][T][T] additive mask (0 / -3e38)
    Norm final_ln;
    std::vector<ClipLayer> layers;
    int* bad = nullptr;
};

// SD-2.1 UNet / ControlNet of the ControlLDM one-step path (ldm/modules/diffusionmodules/openaimodel.py:411-786,
// diffusion/cldm.py:58-292)
struct UResW {        // ResBlock (openaimodel.py:163-272, use_scale_shift_norm = False)
    Norm n1, n2;
    Conv c1, c2, sc;
    bool has_sc = false;
    const float *ew = nullptr, *eb = nullptr;  // emb_layers.1 [cout][temb] fp32; eb already holds in_layers.2's bias + emb_layers.1's bias
    float* bias1 = nullptr;                    // device [cout_pad]: the bias conv1 runs with = eb + ew . silu(emb) for the cached timestep
};
struct UXfW {         // SpatialTransformer with one BasicTransformerBlock (attention.py:205-350, use_linear = True)
    Norm gn, l1, l2, l3;
    Conv pin, pout, qkv, ao, cq, ckv, co, ff1, ff2;
    int heads = 0;
    bf16_t* kc = nullptr;    // [tok_pad][2C]: K | V of the context (set by ir_unet_set_context)
    bf16_t* vtc = nullptr;   // [heads][DV][tok_pad]
};
struct UBlock {
    bool has_res = false, has_xf = false;
    int resample = 0;   // 1: Downsample (stride-2 conv), 2: Upsample (nearest x2 + conv), 3: input_blocks.0 (the first conv)
    UResW res;
    UXfW xf;
    Conv rs;
    int cin = 0, cout = 0;   // channels entering / leaving the block (decoder: cin = h + skip)
    int skip = 0;            // decoder: channels of the skip it pops
};
struct UNetW {
    bool ok = false, ctx_ok = false, control = false;
    int mc = 0, temb = 0, ctx_dim = 0, hd = 0, in_ch = 0, n_levels = 0;
    std::vector<UBlock> in, mid, out;
    std::vector<Conv> zero;   // ControlNet: zero_convs[i] per input block, then middle_block_out
    Norm out_norm;
    Conv out_conv;
    const float *t1w = nullptr, *t1b = nullptr, *t2w = nullptr, *t2b = nullptr;
    float *tsin = nullptr, *th = nullptr, *emb = nullptr, *semb = nullptr;
    float cached_t = -1e30f;
    int n_tok = 0, tok_pad = 0;
};

// the state of the optional per-launch timing (api.cpp's LAUNCH brackets each launch with two events of the pool)
struct ProfRec {
    int cls, kid;
    double flops, bytes;
    hipEvent_t e0, e1;
};
struct Profiler {
    bool on = false;
    int only = -1;   // ir_profile_select: kernel id whose launches alone are bracketed (-1: every launch)
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get() {
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool.push_back(e);
        }
        return pool[used++];
    }
};

// the owner of each list of ir_ctx::own: the context itself, or the binding that a *_configure / set_* call replaces
enum Own { OWN_CTX = 0, OWN_DIT_TABS, OWN_DIT_CTRL_TABS, OWN_DIT_PROMPT, OWN_T5, OWN_CLIP, OWN_LPIPS, OWN_CLIPIQA, OWN_MUSIQ, OWN_MANIQA, OWN_DISTS, OWN_FID, OWN_ILNIQE, OWN_TOPIQ,
           OWN_UNET_TABS, OWN_UNET_CTX = OWN_UNET_TABS + 2, OWN_COUNT = OWN_UNET_CTX + 2 };   // + which: the two UNets' timestep tables / context K-V caches

}  // namespace ir_host

struct ir_ctx {
    int device = 0;
    ir_host::Profiler prof;
    bool fp8 = false;   // ir_set_fp8 / IR_FLAG_FP8: VAE resnet convs with fp8 operands where fp8 weights were uploaded
    uint32_t fp8_mask = IR_FP8_MASK_DEFAULT;   // ir_set_fp8_mask: which parts take fp8 operands when fp8 is on (IR_FP8_BIT_*); default = the guard-chosen set
    bool plain = false; // ir_set_plain_kernels: this context's launches take the older 4-wave kernels (make_run publishes it to the launchers)
    std::string err;
    std::unordered_map<std::string, ir_host::Tensor> t;
    // Every device allocation the context owns besides the tensor table, one list per owner (ir_host::Own). OWN_CTX lives as long as the context; each
    // other list belongs to one binding and is released when that binding is replaced. ir_destroy frees the whole array, so no owner can be forgotten.
    std::vector<void*> own[ir_host::OWN_COUNT];
    int prompt_cap = 0;        // rows (tok_pad) the prompt caches in OWN_DIT_PROMPT were sized for
    int prompt_slots = 0;      // prompts they have room for
    bf16_t *prompt_e16 = nullptr, *prompt_y1 = nullptr, *prompt_y2 = nullptr;   // ir_dit_set_prompts' caption-MLP operands (in OWN_DIT_PROMPT; null until it runs)
    ir_host::SwinModel swin;
    ir_host::VaeModel vae;
    ir_host::DitModel dit;
    ir_host::T5Model t5;
    ir_host::UNetW unet[2];                                  // [0] the diffusion UNet, [1] the ControlNet
    ir_host::ClipTextModel clip;
    // hipGraph cache of ir_pipeline (IR_FLAG_GRAPH): one instantiated graph per exact call signature. `generation` changes whenever
    // device allocations or bindings may have moved (upload with a new size, *_configure, set_prompt), which drops every graph.
    struct GraphKey {
        const void *in, *out, *stage1, *ws, *extra;   // extra + kind: which entry point recorded it (0 ir_pipeline, 1 ir_cldm_pipeline)
        int kind;
        size_t ws_bytes;
        int n, h, w, flags, tile_size, tile_stride;
        float timestep, acp, sf;
        bool operator==(const GraphKey& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    };
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
    unsigned long generation = 0, graphs_generation = 0;
    unsigned long graph_records = 0;   // graphs recorded so far (ir_graph_records)
    hipStream_t cap_stream = nullptr;  // recording happens on a private stream (the caller's may be the legacy default stream, which cannot capture)
    int* shard_flag = nullptr;         // device copy of the overflow flag of the last ir_tiled_encode_part(part 0 / 2) (in OWN_CTX)
    int* attn_fb = nullptr;            // ir_attn_fallback_count: [0] attention launches whose fixed-reference kernel raised its overflow flag (in OWN_CTX)
    bool count_fb = false;             // diagnostic: one counting launch behind every flagged attention (off in the product path)
    double* luma_tab = nullptr;        // ir_metrics_y: the three 256-entry luma tables, filled by ir_init (in OWN_CTX)
    double* niqe_tab = nullptr;        // ir_niqe_stats: three luma tables and v / 255.0, filled by ir_init (in OWN_CTX)
    // ir_lpips: the scaling table, the repacked conv weights [K padded to 32][cout] and copies of the biases / lin heads (in OWN_LPIPS)
    struct Lpips {
        bool ok = false;
        const float *tab = nullptr, *w[5] = {}, *b[5] = {}, *lin[5] = {};
    } lpips;
    // ir_clipiqa: the input table, the repacked conv weights, the folded BatchNorm vectors and copies of the attention pool / text rows (in OWN_CLIPIQA)
    IrClipiqaModel clipiqa;
    // ir_musiq: the input table, the repacked conv weights and transposed linears, copies of the norm vectors and embeddings (in OWN_MUSIQ)
    IrMusiqModel musiq;
    // ir_maniqa: the input table, the transposed linears, copies of the norm vectors, embeddings and relative-position tables (in OWN_MANIQA)
    IrManiqaModel maniqa;
    // ir_topiq: the input table, the repacked convs with their folded BatchNorm, the transposed linears and copies of the norm vectors and embeddings (in OWN_TOPIQ)
    IrTopiqModel topiq;
    // ir_dists: the two input tables, the repacked conv weights and copies of the biases, alpha and beta (in OWN_DISTS)
    IrDistsModel dists;
    // ir_fid_features: the repacked conv weights, the folded BatchNorm vectors and the byte table (in OWN_FID)
    IrFidModel fid;
    // ir_ilniqe_stats / ir_op_dft2_f64: the twiddle tables and copies of the uploaded filter banks, windows and taps (in OWN_ILNIQE)
    IrIlniqeTables ilniqe;
};

namespace ir_host {

inline int fail(ir_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPOK(c, call)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(c, -100, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

inline int pad32(int x) { return (x + 31) & ~31; }
inline std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// entry points that launch without a Run: make the context's GPU current and publish its kernel choice
inline void use_ctx(ir_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    g_ir_plain_kernels = c->plain ? 1 : 0;
}

inline int dev_alloc(ir_ctx* c, std::vector<void*>& list, void** p, size_t bytes) {
    HIPOK(c, hipMalloc(p, (bytes + 255) & ~(size_t)255));
    list.push_back(*p);
    return 0;
}
// Release the buffers of a binding that is being replaced. Kernels that still read them may be in flight on any stream of the
// caller, so the device is drained first (re-binding is a load-time operation, never on the hot path).
inline void release_list(std::vector<void*>& list) {
    if (list.empty()) return;
    (void)hipDeviceSynchronize();
    for (void* p : list) (void)hipFree(p);
    list.clear();
}

// api_image.cpp's part of ir_init (the luma and NIQE tables; nonzero on failure, and the caller destroys the context) and of ir_workspace_bytes
// (true with *bytes when `stage` is one of the image tools', which need no context except for CLIP-IQA's layer counts)
int image_init(ir_ctx* c);
bool image_workspace(ir_ctx* c, int stage, int n, int h, int w, int flags, int tile_size, size_t* bytes);

}  // namespace ir_host
