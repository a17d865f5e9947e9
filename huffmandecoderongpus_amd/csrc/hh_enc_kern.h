// hh_enc_kern.h -- what the encoder's kernels share: the chunk geometry, the
// code table, the workgroup sum, the loads and the image's size
// (csrc/hh_encode.hip: one stream; csrc/hh_encb.hip: blocks, each its own
// stream; csrc/hh_encr.hip: records cut at an offsets list).
#ifndef HH_ENC_KERN_H_
#define HH_ENC_KERN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ENC_TB 256                 // threads per workgroup
#define ENC_PT 16                  // symbols per thread
#define ENC_CH (ENC_TB * ENC_PT)   // symbols per chunk
#define ENC_SCAN_TB 1024

// (lengths: u32 per symbol, 0 = absent; codes: u64, the first stream bit in
// bit 0)
struct EncTab {
    uint64_t code[256];
    uint32_t len[256];
};

__device__ __forceinline__ uint32_t enc_block_sum(uint32_t v, uint32_t *s_w) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) s_w[wv] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (uint32_t i = 0; i < ENC_TB / 64; i++) t += s_w[i];
    return t;
}

// A thread's ENC_PT symbols from i0: one 16-B load when they are all in the
// stream and 16-B aligned (torch tensors are), else byte by byte.
__device__ __forceinline__ void enc_load16(const uint8_t *__restrict__ syms, uint64_t n, uint64_t i0, uint8_t *sy) {
    if (i0 + ENC_PT <= n && (((uintptr_t)(syms + i0)) & 15u) == 0) {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 v = __builtin_nontemporal_load((const u4 *)(syms + i0));
#pragma unroll
        for (uint32_t k = 0; k < ENC_PT; k++) sy[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (uint32_t k = 0; k < ENC_PT; k++) sy[k] = i0 + k < n ? syms[i0 + k] : 0u;
    }
}

// The chunk's image: (sh0 + its bits + 31) / 32 words, sh0 = its first
// bit's position in the output word it starts in.
#define ENC_IMG_WORDS ((31u + ENC_CH * 64u + 31u) / 32u + 1u)

#endif
