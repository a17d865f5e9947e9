// hh_batch_read.hip -- the kernels around k_batch (hh_batch.hip) of a range
// read over a block-coded buffer (hh_decode_blocks_read): byte ranges of the
// uncompressed data become window pieces, one per touched block, which
// k_batch decodes up to the round that fills the window.  HIP (gfx950).  The
// rules are hh_batch_read_algo.h's and hh_batch_plan_algo.h's.
//
// How many pieces the reads have is device data; the host knows only the
// budget P (hbr_budget), so every per-piece array and grid is sized for P
// slots and the slots past the pieces are padding.
//
//   (memset)       the counters ctl
//   k_read_count   a thread per read: the read checked (hbr_read_ok), its
//                  piece count into start[i] (0 for an invalid or empty
//                  read), its copy into reads[i] (zeros for an invalid one:
//                  its offsets never become addresses), its record cleared.
//                  The only kernel that reads the caller's list.  Thread 0
//                  writes the empty summary.
//   k_read_scan    one workgroup: the counts into exclusive first slots, a
//                  tile of 1024 reads per step with the sum carried.  A read
//                  whose pieces would end beyond P is marked HH_ERR_ARG and
//                  gets none; the first such read's first slot, else the
//                  sum, is the number of slots that hold a piece.
//   k_read_fill    a thread per slot s < P: below the total the owning read
//                  by binary search over the first slots (hbr_owner), the
//                  piece's window (hbr_piece), the block's index entry
//                  checked (hbp_item_ok, the output part trivially true) --
//                  the only kernel that reads the index; tmp[s], key[s],
//                  own[s], res[s] untouched.  An entry that breaks a rule and
//                  the slots at or above the total get the empty descriptor:
//                  k_batch walks no round for it.  The workgroup's slots per
//                  bin are counted as k_plan_count does.
//   (k_plan_place, k_batch with n = P)
//   k_read_gather  a thread per slot below the total: the piece's delivered
//                  bytes added to its read's record, a failing piece's
//                  (block ordinal << 8 | -status) folded in by an atomic min
//                  -- no thread walks a read's pieces one after the other.
//   k_read_results a thread per read: d_read_len, d_status; the summary
//                  reduced per workgroup, then atomics; the last workgroup
//                  (a ticket on ctl's done) fills first_failed and
//                  first_status from an atomic min over (read << 32 |
//                  -status), so nothing one workgroup stored is read by
//                  another but through atomics.
// All atomics are ordinary vector atomics on device memory.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hh_batch.h"
#include "hh_batch_algo.h"
#include "hh_batch_plan_algo.h"
#include "hh_batch_read_algo.h"
#include "hh_fsm_kern.h"

#define HBR_TB 256u                  // threads per workgroup (but the scan's)
#define HBR_SCAN_TB 1024u
#define HBR_NONE (~0ull)
static_assert(sizeof(hh_block_read) == 24 && sizeof(hh_batch_item) == 32 && sizeof(BatchDesc) == 56 &&
              sizeof(BatchRes) == 16 && sizeof(hh_batch_summary) == 24, "layouts the kernels assume");
static_assert((HB_CTL_FIRST + 2u) * 4u <= HB_PLAN_CTL_BYTES && HB_CTL_FIRST % 2u == 0, "the counters fit their block");

__global__ __launch_bounds__(HBR_TB) void k_read_count(const hh_block_read *__restrict__ reads, uint32_t m,
                                                       uint64_t n_syms, uint64_t out_bytes, uint64_t B,
                                                       uint64_t *__restrict__ start, hh_block_read *__restrict__ copy,
                                                       uint64_t *__restrict__ rec, int32_t *__restrict__ rstat,
                                                       uint32_t *__restrict__ ctl, hh_batch_summary *__restrict__ sum) {
    const uint32_t i = blockIdx.x * HBR_TB + threadIdx.x;
    if (i == 0) {
        *(uint64_t *)(ctl + HB_CTL_FIRST) = HBR_NONE;
        if (sum) *sum = hh_batch_summary{0, 0, 0xffffffffu, HH_OK, 0};
    }
    if (i >= m) return;
    const hh_block_read r = reads[i];
    const bool ok = hbr_read_ok(r.src_off, r.len, r.dst_off, n_syms, out_bytes) != 0;
    start[i] = ok ? hbr_blocks(r.src_off, r.len, B) : 0u;
    copy[i] = ok ? r : hh_block_read{0, 0, 0};
    rec[2 * (size_t)i] = 0;
    rec[2 * (size_t)i + 1] = HBR_NONE;
    rstat[i] = ok ? HH_OK : HH_ERR_ARG;
}

__global__ __launch_bounds__(HBR_SCAN_TB) void k_read_scan(uint64_t *__restrict__ start, uint32_t m, uint64_t P,
                                                           int32_t *__restrict__ rstat, uint32_t *__restrict__ ctl) {
    __shared__ uint64_t s_w[HBR_SCAN_TB / 64u];
    __shared__ unsigned long long s_total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) s_total = HBR_NONE;
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < m; t0 += HBR_SCAN_TB) {
        const uint64_t i = t0 + tid;
        const uint64_t c = i < m ? start[i] : 0u;
        uint64_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t v = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl = hbr_sat_add(incl, v);
        }
        uint64_t excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0;
        __syncthreads();                                  // (the step before has read s_w; s_total is set)
        if (lane == 63u) s_w[wv] = incl;
        __syncthreads();
        uint64_t woff = 0, tot = 0;
        for (uint32_t v = 0; v < HBR_SCAN_TB / 64u; v++) {
            const uint64_t t = s_w[v];
            if (v < wv) woff = hbr_sat_add(woff, t);
            tot = hbr_sat_add(tot, t);
        }
        const uint64_t st = hbr_sat_add(carry, hbr_sat_add(woff, excl));
        if (i < m) {
            start[i] = st;
            if (!hbr_fits(st, c, P)) {
                rstat[i] = HH_ERR_ARG;
                atomicMin(&s_total, (unsigned long long)st);
            }
        }
        carry = hbr_sat_add(carry, tot);
    }
    __syncthreads();
    if (tid == 0) {
        const uint64_t total = s_total < carry ? (uint64_t)s_total : carry;   // (<= P: the reads before it fit)
        ctl[HB_CTL_TOTAL] = (uint32_t)(total < P ? total : P);
    }
}

__global__ __launch_bounds__(HBR_TB) void k_read_fill(uint32_t P, const uint64_t *__restrict__ start, uint32_t m,
                                                      const hh_block_read *__restrict__ copy,
                                                      const hh_batch_item *__restrict__ index, uint64_t data_bytes,
                                                      uint64_t B, uint64_t RB, BatchDesc *__restrict__ tmp,
                                                      uint8_t *__restrict__ key, BatchRes *__restrict__ res,
                                                      uint32_t *__restrict__ own, uint32_t *__restrict__ ctl) {
    __shared__ uint32_t s_cnt[HBP_BINS];
    const uint32_t tid = threadIdx.x, s = blockIdx.x * HBR_TB + tid;
    if (tid < HBP_BINS) s_cnt[tid] = 0;
    __syncthreads();
    if (s < P) {
        const uint32_t total = ctl[HB_CTL_TOTAL];         // (final: k_read_scan is done)
        BatchDesc d = BatchDesc{0, 0, 0, 0, s, 0, 0, 0};
        uint32_t k = 0, o = 0xffffffffu;
        if (s < total) {
            const uint64_t i = hbr_owner(start, m, s);
            const hh_block_read r = copy[i];
            uint64_t blk, skip, cap, out_off;
            hbr_piece(r.src_off, r.len, r.dst_off, B, s - start[i], &blk, &skip, &cap, &out_off);
            const uint64_t data_off = index[blk].data_off, bits = index[blk].bits;
            o = (uint32_t)i;
            // an entry that breaks a rule never becomes an address
            if (hbp_item_ok(data_off, bits, 0, 0, data_bytes, 0)) {
                d = BatchDesc{data_off, bits, out_off, cap, s, skip, 1u, 0};
                k = hbp_bin(bits, RB);
            } else {
                k = HBP_INVALID;
            }
        }
        tmp[s] = d;
        key[s] = (uint8_t)k;
        own[s] = o;
        res[s] = BatchRes{0, HB_UNTOUCHED};
        atomicAdd(&s_cnt[k & (HBP_BINS - 1u)], 1u);
    }
    __syncthreads();
    if (tid < HBP_BINS && s_cnt[tid]) atomicAdd(&ctl[HB_CTL_CNT + tid], s_cnt[tid]);
}

__global__ __launch_bounds__(HBR_TB) void k_read_gather(uint32_t P, const uint32_t *__restrict__ own,
                                                        const uint64_t *__restrict__ start,
                                                        const BatchRes *__restrict__ res,
                                                        const uint8_t *__restrict__ key, uint64_t *rec,
                                                        const uint32_t *__restrict__ ctl) {
    const uint32_t s = blockIdx.x * HBR_TB + threadIdx.x;
    if (s >= P || s >= ctl[HB_CTL_TOTAL]) return;
    const uint32_t i = own[s];
    const BatchRes r = res[s];
    const bool inv = (key[s] & HBP_INVALID) != 0;
    const int32_t st = inv ? HH_ERR_ARG : r.status == HB_UNTOUCHED ? HH_ERR_INTERNAL : (int32_t)r.status;
    unsigned long long *rc = (unsigned long long *)rec + 2 * (size_t)i;
    if (!inv && r.status != HB_UNTOUCHED && r.len) atomicAdd(rc, (unsigned long long)r.len);
    if (st != HH_OK) atomicMin(rc + 1, (unsigned long long)((s - start[i]) << 8 | (uint64_t)(uint32_t)(-st & 255)));
}

__global__ __launch_bounds__(HBR_TB) void k_read_results(uint32_t m, const uint64_t *__restrict__ rec,
                                                         const int32_t *__restrict__ rstat,
                                                         uint64_t *__restrict__ read_len, int32_t *__restrict__ status,
                                                         hh_batch_summary *sum, uint32_t *ctl) {
    __shared__ uint64_t s_len[HBR_TB / 64u], s_first[HBR_TB / 64u];
    __shared__ uint32_t s_bad[HBR_TB / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, i = blockIdx.x * HBR_TB + tid;
    uint64_t len = 0, first = HBR_NONE;
    uint32_t bad = 0;
    if (i < m) {
        const uint64_t got = rec[2 * (size_t)i], f = rec[2 * (size_t)i + 1];
        const int32_t s = rstat[i] != HH_OK ? rstat[i] : f == HBR_NONE ? HH_OK : -(int32_t)(f & 255u);
        read_len[i] = got;
        status[i] = s;
        len = s == HH_OK ? got : 0u;                      // (the summary's total: the reads that succeeded)
        if (s != HH_OK) {
            bad = 1;
            first = (uint64_t)i << 32 | (uint32_t)(-s);
        }
    }
    if (!sum) return;                                     // (uniform: a kernel argument)
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        len += __shfl_xor(len, o, 64);
        bad += __shfl_xor(bad, o, 64);
        const uint64_t f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        s_len[wv] = len;
        s_bad[wv] = bad;
        s_first[wv] = first;
    }
    __syncthreads();
    if (tid != 0) return;
    for (uint32_t v = 1; v < HBR_TB / 64u; v++) {
        len += s_len[v];
        bad += s_bad[v];
        first = s_first[v] < first ? s_first[v] : first;
    }
    unsigned long long *gfirst = (unsigned long long *)(ctl + HB_CTL_FIRST);
    if (len) atomicAdd((unsigned long long *)&sum->total_len, (unsigned long long)len);
    if (bad) {
        atomicAdd(&sum->n_failed, bad);
        atomicMin(gfirst, (unsigned long long)first);
    }
    // the last workgroup to get here sees every workgroup's minimum
    __threadfence();
    if (atomicAdd(&ctl[HB_CTL_DONE], 1u) != gridDim.x - 1u) return;
    __threadfence();
    const uint64_t ff = atomicMin(gfirst, (unsigned long long)HBR_NONE);   // (an atomic read)
    if (ff != HBR_NONE) {
        sum->first_failed = (uint32_t)(ff >> 32);
        sum->first_status = -(int32_t)(uint32_t)ff;
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static size_t up8(size_t x) { return (x + 7u) & ~(size_t)7u; }

size_t read_ws_bytes(uint64_t m, uint32_t P) {
    return (size_t)P * (2 * sizeof(BatchDesc) + sizeof(BatchRes)) + (size_t)m * (8 + sizeof(hh_block_read) + 16) +
           up8((size_t)P * 4) + up8((size_t)m * 4) + HB_PLAN_CTL_BYTES + (((size_t)P + 255u) & ~(size_t)255u);
}

void read_ws_carve(ReadWs *w, void *d_ws, uint64_t m, uint32_t P) {
    uint8_t *p = (uint8_t *)d_ws;
    w->desc = (BatchDesc *)p;       p += (size_t)P * sizeof(BatchDesc);
    w->tmp = (BatchDesc *)p;        p += (size_t)P * sizeof(BatchDesc);
    w->res = (BatchRes *)p;         p += (size_t)P * sizeof(BatchRes);
    w->start = (uint64_t *)p;       p += (size_t)m * 8;
    w->reads = (hh_block_read *)p;  p += (size_t)m * sizeof(hh_block_read);
    w->rec = (uint64_t *)p;         p += (size_t)m * 16;
    w->own = (uint32_t *)p;         p += up8((size_t)P * 4);
    w->rstat = (int32_t *)p;        p += up8((size_t)m * 4);
    w->ctl = (uint32_t *)p;         p += HB_PLAN_CTL_BYTES;
    w->key = p;
}

int read_count_enqueue(const ReadWs *w, uint64_t n_syms, uint64_t block_syms, const hh_block_read *d_reads,
                       uint32_t m, uint32_t P, uint64_t out_bytes, hh_batch_summary *d_summary, hipStream_t st) {
    if (m == 0 || P == 0 || block_syms == 0) return HH_ERR_INTERNAL;
    const uint32_t gm = (uint32_t)(((uint64_t)m + HBR_TB - 1u) / HBR_TB);
    FS_OK(hipMemsetAsync(w->ctl, 0, HB_PLAN_CTL_BYTES, st));
    hipLaunchKernelGGL(k_read_count, dim3(gm), dim3(HBR_TB), 0, st, d_reads, m, n_syms, out_bytes, block_syms,
                       w->start, w->reads, w->rec, w->rstat, w->ctl, d_summary);
    FS_OK(hipGetLastError());
    hipLaunchKernelGGL(k_read_scan, dim3(1), dim3(HBR_SCAN_TB), 0, st, w->start, m, (uint64_t)P, w->rstat, w->ctl);
    FS_OK(hipGetLastError());
    return HH_OK;
}

int read_plan_enqueue(const ReadWs *w, const hh_batch_item *d_index, uint64_t data_bytes, uint64_t n_syms,
                      uint64_t block_syms, const hh_block_read *d_reads, uint32_t m, uint32_t P, uint64_t out_bytes,
                      uint64_t round_bits, hh_batch_summary *d_summary, hipStream_t st) {
    if (round_bits == 0) return HH_ERR_INTERNAL;
    const int rc = read_count_enqueue(w, n_syms, block_syms, d_reads, m, P, out_bytes, d_summary, st);
    if (rc != HH_OK) return rc;
    const uint32_t gp = (uint32_t)(((uint64_t)P + HBR_TB - 1u) / HBR_TB);
    hipLaunchKernelGGL(k_read_fill, dim3(gp), dim3(HBR_TB), 0, st, P, (const uint64_t *)w->start, m,
                       (const hh_block_read *)w->reads, d_index, data_bytes, block_syms, round_bits, w->tmp, w->key,
                       w->res, w->own, w->ctl);
    FS_OK(hipGetLastError());
    return HH_OK;
}

int read_results_enqueue(const ReadWs *w, uint32_t m, uint32_t P, uint64_t *d_read_len, int32_t *d_status,
                         hh_batch_summary *d_summary, hipStream_t st) {
    const uint32_t gm = (uint32_t)(((uint64_t)m + HBR_TB - 1u) / HBR_TB);
    const uint32_t gp = (uint32_t)(((uint64_t)P + HBR_TB - 1u) / HBR_TB);
    hipLaunchKernelGGL(k_read_gather, dim3(gp), dim3(HBR_TB), 0, st, P, (const uint32_t *)w->own,
                       (const uint64_t *)w->start, (const BatchRes *)w->res, (const uint8_t *)w->key, w->rec,
                       (const uint32_t *)w->ctl);
    FS_OK(hipGetLastError());
    hipLaunchKernelGGL(k_read_results, dim3(gm), dim3(HBR_TB), 0, st, m, (const uint64_t *)w->rec,
                       (const int32_t *)w->rstat, d_read_len, d_status, d_summary, w->ctl);
    FS_OK(hipGetLastError());
    return HH_OK;
}
