// hh_batch_plan.hip -- the kernels around k_batch (hh_batch.hip) of a batch
// whose items are a device array (hh_decode_batch_device_items): what
// batch_decode does on the host per call -- check the items, order them
// longest first, write the descriptors, mark the results untouched, read the
// results back -- done on the device, in the order of the caller's stream.
// HIP (gfx950).  The rules are hh_batch_plan_algo.h's.
//
//   (memset)      the counters ctl: cnt[64] streams per bin, cur[64] the bins'
//                 placement cursors, done: the results' workgroups finished
//   k_plan_count  a thread per item: the item checked (hbp_key), its
//                 descriptor -- the empty one for an invalid item -- into tmp[i],
//                 its key byte into key[i], res[i] marked untouched; the
//                 workgroup's streams per bin counted in LDS, then one atomic
//                 add per occupied bin on cnt.  The only kernel that reads the
//                 caller's list.  Thread 0 writes the empty summary.
//   k_plan_place  a thread per item: every workgroup turns cnt into the bins'
//                 starts (hbp_start, a lane per bin), counts its streams per
//                 bin in LDS again (an LDS atomic gives a stream its rank in
//                 the workgroup's share), reserves that share with one atomic
//                 add per occupied bin on cur, and moves tmp[i] to its place
//                 in the list.
//   (k_batch)
//   k_batch_results  a thread per stream: out_len, status (HH_ERR_ARG for an
//                 invalid item, HH_ERR_INTERNAL for a slot k_batch left
//                 untouched); the summary reduced per workgroup, then one
//                 atomic add for the total, one for the failures, one atomic
//                 min for the first of them; the last workgroup to finish
//                 (a ticket on ctl's done) fills first_status.
//
// The counting sort uses atomic adds on per-bin cursors, not per-workgroup
// count slabs: the order inside a bin then depends on which workgroup adds
// first, but k_batch's results do not depend on the list's order at all
// (every stream is decoded from its own descriptor into its own output and
// result slot), only its tail does, and streams of one bin cost the same
// rounds.  The slabs would need a scan over workgroups (a third kernel, or a
// single workgroup walking nwg x 64 counts) to buy an order nothing reads.
// All atomics are ordinary vector atomics on device memory.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hh_batch.h"
#include "hh_batch_algo.h"
#include "hh_batch_plan_algo.h"
#include "hh_fsm_kern.h"

#define HBP_TB 256u                  // threads per workgroup of the three kernels
#define HBP_CNT HB_CTL_CNT           // ctl (u32 words): cnt[HBP_BINS]
#define HBP_CUR HB_CTL_CUR           //                  cur[HBP_BINS]
#define HBP_DONE HB_CTL_DONE         //                  done
static_assert(HBP_CUR == HBP_BINS && HBP_DONE == 2u * HBP_BINS, "ctl's layout (hh_batch.h) is for HBP_BINS bins");
static_assert((HBP_DONE + 1u) * 4u <= HB_PLAN_CTL_BYTES, "the plan's counters fit their block");
static_assert(sizeof(hh_batch_item) == 32 && sizeof(BatchDesc) == 56 && sizeof(BatchRes) == 16 &&
              sizeof(hh_batch_summary) == 24, "layouts the kernels assume");

__global__ __launch_bounds__(HBP_TB) void k_plan_count(const hh_batch_item *__restrict__ items, uint32_t n,
                                                       uint64_t data_bytes, uint64_t out_bytes, uint64_t RB,
                                                       BatchDesc *__restrict__ tmp, uint8_t *__restrict__ key,
                                                       BatchRes *__restrict__ res, uint32_t *__restrict__ ctl,
                                                       hh_batch_summary *__restrict__ sum) {
    __shared__ uint32_t s_cnt[HBP_BINS];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * HBP_TB + tid;
    if (tid < HBP_BINS) s_cnt[tid] = 0;
    __syncthreads();
    if (i < n) {
        const hh_batch_item it = items[i];
        const uint32_t k = hbp_key(it.data_off, it.bits, it.out_off, it.cap, data_bytes, out_bytes, RB);
        const bool ok = !(k & HBP_INVALID);
        // an invalid item's offsets are never copied: they must not become addresses
        tmp[i] = ok ? BatchDesc{it.data_off, it.bits, it.out_off, it.cap, i, 0, 0, 0} : BatchDesc{0, 0, 0, 0, i, 0, 0, 0};
        key[i] = (uint8_t)k;
        res[i] = BatchRes{0, HB_UNTOUCHED};
        atomicAdd(&s_cnt[k & (HBP_BINS - 1u)], 1u);
    }
    __syncthreads();
    if (tid < HBP_BINS && s_cnt[tid]) atomicAdd(&ctl[HBP_CNT + tid], s_cnt[tid]);
    if (i == 0 && sum) *sum = hh_batch_summary{0, 0, 0xffffffffu, HH_OK, 0};
}

__global__ __launch_bounds__(HBP_TB) void k_plan_place(const BatchDesc *__restrict__ tmp,
                                                       const uint8_t *__restrict__ key, uint32_t n,
                                                       uint32_t *__restrict__ ctl, BatchDesc *__restrict__ desc) {
    __shared__ uint32_t s_cnt[HBP_BINS], s_loc[HBP_BINS], s_base[HBP_BINS];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * HBP_TB + tid;
    if (tid < HBP_BINS) {
        s_cnt[tid] = ctl[HBP_CNT + tid];                  // (final: k_plan_count is done)
        s_loc[tid] = 0;
    }
    __syncthreads();
    uint32_t bin = 0, rank = 0;
    if (i < n) {
        bin = key[i] & (HBP_BINS - 1u);
        rank = atomicAdd(&s_loc[bin], 1u);
    }
    __syncthreads();
    if (tid < HBP_BINS)
        s_base[tid] = hbp_start(s_cnt, tid) + (s_loc[tid] ? atomicAdd(&ctl[HBP_CUR + tid], s_loc[tid]) : 0u);
    __syncthreads();
    if (i < n) {
        const uint32_t at = s_base[bin] + rank;
        if (at < n) desc[at] = tmp[i];                    // (always: the counts are of these very keys)
    }
}

__global__ __launch_bounds__(HBP_TB) void k_batch_results(const BatchRes *__restrict__ res,
                                                          const uint8_t *__restrict__ key, uint32_t n,
                                                          uint64_t *__restrict__ out_len, int32_t *__restrict__ status,
                                                          hh_batch_summary *sum, uint32_t *ctl) {
    __shared__ uint64_t s_len[HBP_TB / 64u];
    __shared__ uint32_t s_bad[HBP_TB / 64u], s_first[HBP_TB / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, i = blockIdx.x * HBP_TB + tid;
    uint64_t len = 0;
    uint32_t bad = 0, first = 0xffffffffu;
    if (i < n) {
        const BatchRes r = res[i];
        const bool inv = (key[i] & HBP_INVALID) != 0;
        const int32_t s = inv ? HH_ERR_ARG : r.status == HB_UNTOUCHED ? HH_ERR_INTERNAL : (int32_t)r.status;
        len = inv ? 0 : r.len;
        out_len[i] = len;
        status[i] = s;
        if (s != HH_OK && s != HH_ERR_CAPACITY) len = 0;  // (the summary's total: decoded streams only)
        if (s != HH_OK) {
            bad = 1;
            first = i;
        }
    }
    if (!sum) return;                                     // (uniform: a kernel argument)
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        len += __shfl_xor(len, o, 64);
        bad += __shfl_xor(bad, o, 64);
        const uint32_t f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_len[wv] = len;
        s_bad[wv] = bad;
        s_first[wv] = first;
    }
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t v = 1; v < HBP_TB / 64u; v++) {
        len += s_len[v];
        bad += s_bad[v];
        first = s_first[v] < first ? s_first[v] : first;
    }
    if (len) atomicAdd((unsigned long long *)&sum->total_len, (unsigned long long)len);
    if (bad) {
        atomicAdd(&sum->n_failed, bad);
        atomicMin(&sum->first_failed, first);
    }
    // the last workgroup to get here sees every workgroup's minimum
    __threadfence();
    if (atomicAdd(&ctl[HBP_DONE], 1u) != gridDim.x - 1u) return;
    __threadfence();
    const uint32_t ff = atomicMin(&sum->first_failed, 0xffffffffu);   // (an atomic read)
    if (ff < n) {
        const BatchRes r = res[ff];
        sum->first_status = (key[ff] & HBP_INVALID) ? HH_ERR_ARG
                            : r.status == HB_UNTOUCHED ? HH_ERR_INTERNAL : (int32_t)r.status;
    }
}

int batch_plan_enqueue(const hh_batch_item *d_items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                       uint64_t round_bits, BatchDesc *desc, BatchRes *res, BatchDesc *tmp, uint8_t *key,
                       uint32_t *ctl, hh_batch_summary *d_summary, hipStream_t st) {
    if (n == 0 || round_bits == 0) return HH_ERR_INTERNAL;
    const uint32_t grid = (uint32_t)(((uint64_t)n + HBP_TB - 1u) / HBP_TB);
    FS_OK(hipMemsetAsync(ctl, 0, HB_PLAN_CTL_BYTES, st));
    hipLaunchKernelGGL(k_plan_count, dim3(grid), dim3(HBP_TB), 0, st, d_items, n, data_bytes, out_bytes, round_bits,
                       tmp, key, res, ctl, d_summary);
    FS_OK(hipGetLastError());
    return batch_place_enqueue(tmp, key, n, ctl, desc, st);
}

int batch_place_enqueue(const BatchDesc *tmp, const uint8_t *key, uint32_t n, uint32_t *ctl, BatchDesc *desc,
                        hipStream_t st) {
    const uint32_t grid = (uint32_t)(((uint64_t)n + HBP_TB - 1u) / HBP_TB);
    hipLaunchKernelGGL(k_plan_place, dim3(grid), dim3(HBP_TB), 0, st, tmp, key, n, ctl, desc);
    FS_OK(hipGetLastError());
    return HH_OK;
}

int batch_results_enqueue(const BatchRes *res, const uint8_t *key, uint32_t n, uint64_t *d_out_len,
                          int32_t *d_status, hh_batch_summary *d_summary, uint32_t *ctl, hipStream_t st) {
    const uint32_t grid = (uint32_t)(((uint64_t)n + HBP_TB - 1u) / HBP_TB);
    hipLaunchKernelGGL(k_batch_results, dim3(grid), dim3(HBP_TB), 0, st, res, key, n, d_out_len, d_status, d_summary,
                       ctl);
    FS_OK(hipGetLastError());
    return HH_OK;
}

int batch_summary_clear(hh_batch_summary *d_summary, hipStream_t st) {
    FS_OK(hipMemsetAsync(d_summary, 0, sizeof(*d_summary), st));
    FS_OK(hipMemsetAsync(&d_summary->first_failed, 0xff, sizeof(d_summary->first_failed), st));
    return HH_OK;
}
