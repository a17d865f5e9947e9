// hh_hist_kern.h -- the byte-histogram kernels (csrc/hh_hist.hip launches
// them; tools/ubench/ub_hist.hip sweeps their parameters).
//
//   k_hist<COPIES>  persistent grid (a multiple of the CU count, not one
//                   workgroup per chunk): 16-B nontemporal loads in a
//                   grid-stride loop over the 16-B aligned body of the input,
//                   every byte one no-return LDS atomic add on a u32 counter
//                   of the workgroup's histogram; the bytes before the first
//                   and after the last 16-B boundary (at most 15 each) are
//                   counted one at a time by workgroup 0.  Then each
//                   workgroup stores its 256 sums (plain stores) to its row
//                   of the [grid][256] slab.
//   k_hist_sum      8 workgroups: the slab's columns summed into 256 u64.
// No global atomics: the counts are exact and independent of the order the
// workgroups run in.
//
// LDS layout: COPIES histograms per workgroup, lane l adds into copy
// l % COPIES.  Text is skewed (a space is one byte in six of kjv), and lanes
// that add to one counter serialise; with COPIES copies at most 64 / COPIES
// lanes of a wave share a counter.  A copy is HIST_STRIDE = 257 words, not
// 256, so that the same byte value in copy c lies in bank (value + c) % 32:
// the lanes that hit the hot value in different copies hit different banks.
#ifndef HH_HIST_KERN_H_
#define HH_HIST_KERN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define HIST_TB 256            // threads per workgroup
#define HIST_STRIDE 257u       // words per LDS copy (256 counters + 1: bank skew)
#define HIST_SUM_WGS 8         // k_hist_sum: workgroups, 32 columns each
#define HIST_SUM_TB 1024

typedef uint32_t hist_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void hist_add16(uint32_t *__restrict__ h, const hist_u4 v) {
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t x = v[w];
        atomicAdd(&h[x & 0xffu], 1u);
        atomicAdd(&h[(x >> 8) & 0xffu], 1u);
        atomicAdd(&h[(x >> 16) & 0xffu], 1u);
        atomicAdd(&h[x >> 24], 1u);
    }
}

// syms: n bytes at any alignment.  slab: gridDim.x rows of 256 u32.
// A workgroup counts at most ceil(nvec / (grid * HIST_TB)) * HIST_TB 16-B
// vectors plus 30 single bytes; the launcher keeps that below 2^32 bytes
// (hh_hist.hip: HIST_WG_MAX_BYTES), so no u32 counter can overflow.
template <int COPIES>
__global__ __launch_bounds__(HIST_TB) void k_hist(const uint8_t *__restrict__ syms, uint64_t n,
                                                  uint32_t *__restrict__ slab) {
    __shared__ uint32_t s_h[COPIES * HIST_STRIDE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < COPIES * HIST_STRIDE; i += HIST_TB) s_h[i] = 0u;
    __syncthreads();
    uint32_t *h = s_h + (tid % COPIES) * HIST_STRIDE;
    // [0, head) single bytes, nvec aligned 16-B vectors, then tail < 16 bytes
    uint64_t head = (16u - (uint32_t)((uintptr_t)syms & 15u)) & 15u;
    if (head > n) head = n;
    const uint64_t nvec = (n - head) >> 4;
    const uint32_t tail = (uint32_t)(n - head - (nvec << 4));
    if (blockIdx.x == 0) {
        if (tid < (uint32_t)head) atomicAdd(&h[syms[tid]], 1u);
        if (tid >= 32u && tid - 32u < tail) atomicAdd(&h[syms[head + (nvec << 4) + (tid - 32u)]], 1u);
    }
    const hist_u4 *__restrict__ body = (const hist_u4 *)(syms + head);
    const uint64_t stride = (uint64_t)gridDim.x * HIST_TB;
    uint64_t v = (uint64_t)blockIdx.x * HIST_TB + tid;
    // four loads in flight per lane
    for (; v + 3 * stride < nvec; v += 4 * stride) {
        const hist_u4 a = __builtin_nontemporal_load(body + v);
        const hist_u4 b = __builtin_nontemporal_load(body + v + stride);
        const hist_u4 c = __builtin_nontemporal_load(body + v + 2 * stride);
        const hist_u4 d = __builtin_nontemporal_load(body + v + 3 * stride);
        hist_add16(h, a);
        hist_add16(h, b);
        hist_add16(h, c);
        hist_add16(h, d);
    }
    for (; v < nvec; v += stride) hist_add16(h, __builtin_nontemporal_load(body + v));
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int c = 0; c < COPIES; c++) t += s_h[c * HIST_STRIDE + tid];
    slab[(uint64_t)blockIdx.x * 256u + tid] = t;
}

// counts[b] = sum over rows of slab[row][b].  Workgroup w sums columns
// [32 w, 32 w + 32): 32 row groups of 32 lanes, each a 128-B row segment per
// load, then the row groups' sums added through LDS.
__global__ __launch_bounds__(HIST_SUM_TB) void k_hist_sum(const uint32_t *__restrict__ slab, uint32_t rows,
                                                          uint64_t *__restrict__ counts) {
    __shared__ uint64_t s_p[32][33];
    const uint32_t tid = threadIdx.x, col = tid & 31u, rg = tid >> 5;
    const uint32_t b = blockIdx.x * 32u + col;
    uint64_t acc = 0;
    for (uint32_t r = rg; r < rows; r += 32u) acc += slab[(uint64_t)r * 256u + b];
    s_p[rg][col] = acc;
    __syncthreads();
    if (tid < 32u) {
        uint64_t t = 0;
#pragma unroll
        for (uint32_t i = 0; i < 32u; i++) t += s_p[i][tid];
        counts[b] = t;
    }
}

#endif
