// The cache of encoded captions behind ir_t5_encode_prompts (prompts typed as text inside a run; no reference counterpart - the reference
// encodes captions offline, tools/extract_caption.py:150-163, and saves `caption_emb.to(torch.float16)` with an int16 mask). Two memory-bound
// kernels: the store narrows the encoder's fp32 rows into a cache slot, the gather widens the slots of a batch into the block
// ir_dit_set_prompts takes. Neither reads outside its arguments whatever the slot indices are.
#include <hip/hip_runtime.h>
#include "common.h"
#include "kernels.h"

// fp32 -> fp16 bits, round to nearest even, overflow to infinity, subnormal results kept (the conversion instruction's IEEE behaviour: the
// bits of torch's tensor.to(torch.float16))
__device__ __forceinline__ uint32_t pack2h(float a, float b) {
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    return (uint32_t)__builtin_bit_cast(unsigned short, ha) | ((uint32_t)__builtin_bit_cast(unsigned short, hb) << 16);
}
__device__ __forceinline__ float h2f(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16); }

// dst (fp16 or fp32, `nv` groups of 4 elements) = src; the first `nm` threads also copy one mask entry each (1.0 without a source mask)
__global__ __launch_bounds__(256) void prompt_cache_store_kernel(const float* __restrict__ src, const float* __restrict__ mask_src, void* __restrict__ dst,
                                                                float* __restrict__ mask_dst, int fp16, long nv, long nm) {
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    for (long i = t0; i < nv; i += step) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i * 4);
        if (fp16)
            *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(dst) + i * 4) = make_uint2(pack2h(v[0], v[1]), pack2h(v[2], v[3]));
        else
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dst) + i * 4) = v;
    }
    for (long i = t0; i < nm; i += step) mask_dst[i] = mask_src ? mask_src[i] : 1.f;
}

// one image per blockIdx.y: its T * D embedding elements (nv groups of 4) and, in the image's first block, its T bias entries
__global__ __launch_bounds__(256) void prompt_gather_kernel(const void* __restrict__ cache, const float* __restrict__ cache_mask, int fp16, int n_slots,
                                                           const int* __restrict__ slots, const float* __restrict__ fixed_embeds,
                                                           const float* __restrict__ fixed_mask, float* __restrict__ embeds_out,
                                                           float* __restrict__ bias_out, int T, long nv, int* __restrict__ bad_slot) {
    const int img = blockIdx.y;
    int slot = slots[img];
    if (slot >= n_slots) {   // never read outside the cache: the fixed prompt, and the caller's status word says so
        if (bad_slot && blockIdx.x == 0 && threadIdx.x == 0) *bad_slot = 1;
        slot = -1;
    }
    float* out = embeds_out + (long)img * nv * 4;
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (slot < 0) {
        for (long i = t0; i < nv; i += step) *reinterpret_cast<f32x4*>(out + i * 4) = *reinterpret_cast<const f32x4*>(fixed_embeds + i * 4);
    } else if (fp16) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(cache) + (long)slot * nv * 4;
        for (long i = t0; i < nv; i += step) {
            const uint2 w = *reinterpret_cast<const uint2*>(src + i * 4);
            const f32x4 v = {h2f(w.x & 0xffffu), h2f(w.x >> 16), h2f(w.y & 0xffffu), h2f(w.y >> 16)};
            *reinterpret_cast<f32x4*>(out + i * 4) = v;
        }
    } else {
        const float* src = reinterpret_cast<const float*>(cache) + (long)slot * nv * 4;
        for (long i = t0; i < nv; i += step) *reinterpret_cast<f32x4*>(out + i * 4) = *reinterpret_cast<const f32x4*>(src + i * 4);
    }
    if (blockIdx.x == 0) {
        const float* m = slot < 0 ? fixed_mask : cache_mask + (long)slot * T;
        for (int t = threadIdx.x; t < T; t += 256) bias_out[(long)img * T + t] = m[t];
    }
}

int ir_launch_prompt_cache_store(const float* src, const float* mask_src, void* cache, float* cache_mask, int fp16, int slot0, int b, int T, int D,
                                 hipStream_t s) {
    if (b <= 0 || T <= 0 || D <= 0 || (D & 3) || slot0 < 0) return -2;
    const long per = (long)T * D, nv = (long)b * per / 4, nm = (long)b * T;
    void* dst = fp16 ? (void*)(reinterpret_cast<unsigned short*>(cache) + (long)slot0 * per) : (void*)(reinterpret_cast<float*>(cache) + (long)slot0 * per);
    long blocks = (nv + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(prompt_cache_store_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, mask_src, dst, cache_mask + (long)slot0 * T, fp16, nv, nm);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int ir_launch_prompt_gather(const void* cache, const float* cache_mask, int fp16, int n_slots, const int* slots, const float* fixed_embeds,
                            const float* fixed_mask, float* embeds_out, float* bias_out, int n, int T, int D, int* bad_slot, hipStream_t s) {
    if (n <= 0 || n > 65535 || T <= 0 || D <= 0 || (D & 3) || n_slots < 0) return -2;
    const long nv = (long)T * D / 4;
    long blocks = (nv + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(prompt_gather_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, cache, cache_mask, fp16, n_slots, slots, fixed_embeds,
                       fixed_mask, embeds_out, bias_out, T, nv, bad_slot);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
