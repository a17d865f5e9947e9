// hh_batch.hip -- the batched decode: n independent streams of one code in a
// single launch (hh_decode_batch_device).  HIP (gfx950).
//
// k_batch: a workgroup of W waves takes streams from the descriptor list
// (longest first: sorted by the host, or bin-ordered on the device by
// hh_batch_plan.hip for hh_decode_batch_device_items; workgroup b takes
// entries b, b + grid, ...: nothing waits on another workgroup) and decodes each in
// rounds of W tiles -- 64 W regions of S bits, lane = region -- by the rules
// of hh_batch_algo.h: guess, count, fix rounds, scan, emission, copy-out.
// The state entering the next round and the output base are carried from
// round to round, so a stream needs no second kernel and no scan over tiles.
//
// LDS (dynamic only, from address 0: hh_fsm_kern.h's rule):
//   the emission tables et, er, b1, tsym (emf_tab_bytes; the count pass walks
//   them too: an entry carries the symbol count and the next state, and the
//   count table would not fit beside them for a byte alphabet)
//   the round's payload, a row of SW (+ 1 when SW is even) words per region
//   wx[16] waves' exit states, wt[16] waves' counts, chg[3] fix-round flags
//   the round's staging: its symbols at their output address mod 16
//
// Window pieces (hh_decode_blocks_read; hh_batch_read.hip makes them): a
// descriptor with `win` set wants the stream's symbols [skip, skip + cap)
// only.  Rounds before the window are counted and not emitted, of the others
// the window's bytes alone are copied out (hb_window), and the piece ends
// after the round that fills the window: later rounds are neither loaded nor
// walked.  Its result is the bytes delivered, HH_ERR_FORMAT when the stream
// ended before the window was full.
//
// Output edges: neighbouring streams' outputs may share a dword (any out_off,
// exact capacities) and another workgroup writes the neighbour, so the
// copy-out stores whole 16-byte blocks only where all 16 bytes are this
// round's, and single bytes elsewhere: never a byte it does not own.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hh_batch.h"
#include "hh_batch_algo.h"
#include "hh_fsm_kern.h"

__global__ __launch_bounds__(64 * HB_WMAX) void k_batch(const uint8_t *__restrict__ data,
                                                        const BatchDesc *__restrict__ desc, BatchRes *__restrict__ res,
                                                        uint8_t *__restrict__ out, FsmTab tab, BatchGeo geo) {
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t ns = geo.ns, K = geo.K, r = geo.r, S = geo.S, G = geo.G, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t W = geo.W, SW = S / 32u, RW = hb_row_words(S);
    const uint32_t er_off = (ns << HH_FSM_ET_LG(K)) * 8u;
    uint32_t *s_b1 = (uint32_t *)(smem + er_off + (r ? (ns << r) * 8u : 0u));
    uint8_t *s_ts = (uint8_t *)(s_b1 + 2 * ns);
    lds_fill16(smem, tab.et, er_off);
    for (uint32_t i = tid; r && i < (ns << r); i += blockDim.x) ((uint64_t *)(smem + er_off))[i] = tab.er[i];
    for (uint32_t i = tid; i < 2 * ns; i += blockDim.x) s_b1[i] = tab.b1[i];
    for (uint32_t i = tid; i < ns; i += blockDim.x) s_ts[i] = tab.tsym[i];
    const hb_view F = {(const uint64_t *)smem, (const uint64_t *)(smem + er_off), s_b1, s_ts, K, r, S};
    uint32_t *pay = (uint32_t *)(smem + geo.pay_off);
    uint32_t *wx = (uint32_t *)(smem + geo.misc_off), *wt = wx + HB_WMAX, *chg = wt + HB_WMAX;
    uint8_t *stg = smem + geo.stg_off;
    const bool lds0 = lds_base_is_zero(smem);
    const uint32_t jr = wv * 64u + lane;                  // the lane's region of a round
    const uint64_t RB = (uint64_t)HB_NR * W * S;          // a round's bits

    for (uint32_t it = blockIdx.x; it < geo.n; it += gridDim.x) {
        const uint64_t data_off = uni64(desc[it].data_off), bits = uni64(desc[it].bits);
        const uint64_t out_off = uni64(desc[it].out_off), cap = uni64(desc[it].cap), idx = uni64(desc[it].idx);
        // a window piece wants the stream's symbols [skip, skip + cap) only (else skip is 0)
        const uint64_t skip = uni64(desc[it].skip);
        const bool win = __builtin_amdgcn_readfirstlane((int)desc[it].win) != 0;
        const uint32_t *g = (const uint32_t *)(data + data_off);
        const uint64_t nwords = (bits + 31u) / 32u, rounds = win && !cap ? 0u : (bits + RB - 1u) / RB;
        uint64_t base = 0, got = 0;                       // symbols before the round; bytes delivered
        uint32_t carry = 0, fail = lds0 ? 0u : 1u;        // the state entering the round
        for (uint64_t rd = 0; rd < rounds; rd++) {
            const uint64_t R0 = rd * RB, R = R0 + (uint64_t)jr * S;
            // the round's payload: every lane its region's words into its row
            // (loads past the stream's words give 0, never read as stream bits)
            const __amdgpu_buffer_rsrc_t rs = fs_rsrc(g, R0 / 32u, nwords);
            __syncthreads();                              // the round before has read its rows and its staging
            uint32_t *row = pay + jr * RW;
#pragma unroll 4
            for (uint32_t k = 0; k < SW; k++) row[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(4u * (jr * SW + k)), 0, 0);
            if (tid == 0) chg[0] = 0;
            __syncthreads();
            int whole, at_end;
            const uint32_t nb = hb_span(R, S, bits, &whole, &at_end);
            hb_bits b;
            uint32_t ent = carry, x, n;
            if (jr > 0) {
                ent = 0;
                if (G && nb) {
                    hb_bits_init(&b, pay + (jr - 1u) * RW, S - G);
                    ent = hb_guess(&F, &b, G);
                }
            }
            hb_no_sink none;
            hb_bits_init(&b, row, 0);
            x = hb_region(&F, &b, nb, whole, at_end, ent, none, &n);
            // fix rounds: until no lane's entry differs from its predecessor's exit
            uint32_t c3 = 0, fr = 0;
            for (;; fr++) {
                if (lane == 63u) wx[wv] = x;
                const uint32_t c3n = c3 == 2u ? 0u : c3 + 1u;
                if (tid == 0) chg[c3n] = 0;
                __syncthreads();
                uint32_t pred = shfl_up1(x);
                if (lane == 0) pred = wv ? wx[wv - 1u] : carry;
                const int again = hb_fix(jr, nb, pred, &ent);
                if (again) {
                    hb_bits_init(&b, row, 0);
                    x = hb_region(&F, &b, nb, whole, at_end, ent, none, &n);
                }
                if (__builtin_amdgcn_ballot_w64(again != 0) != 0 && lane == 0) chg[c3] = 1u;
                __syncthreads();
                const uint32_t any = chg[c3];
                c3 = c3n;
                if (!any) break;
                if (fr >= HB_FIX_BOUND(W)) { fail = 1u; break; }   // (cannot happen: hh_batch_algo.h)
            }
            const uint32_t carry_next = wx[W - 1u];        // (the last fix round changed nothing: wx is final)
            // scan
            const uint32_t incl = (uint32_t)wave_incl_scan((int32_t)n);
            if (lane == 63u) wt[wv] = incl;
            __syncthreads();
            uint32_t woff = 0, tot = 0;
            for (uint32_t v = 0; v < W; v++) {
                const uint32_t t = wt[v];
                woff += v < wv ? t : 0u;
                tot += t;
            }
            const uint32_t L = woff + incl - n;
            // emission into the staging, at the output's address mod 16: the
            // round's byte t at a0 + t.  ga is the address of t = 0, which for
            // a round that starts before the window is no address of the
            // buffer (unsigned arithmetic; only the window's bytes, from
            // `from` on, are ever stored)
            const uintptr_t ga = (uintptr_t)out + out_off + base - skip;
            const uint32_t a0 = (uint32_t)(ga & 15u);
            uint32_t from;
            const uint32_t keep = hb_window(base, tot, skip, cap, &from);
            if (a0 + tot + 8u > geo.stg_bytes) fail = 1u;       // (the host sized it for the most a round holds)
            if (!fail && keep) {
                if (tid == 0) *(uint32_t *)(stg + ((a0 + tot) & ~3u)) = 0u;   // the last, partial dword: ORs only
                BatchSink sink;
                sink.init(smem, geo.stg_off + a0 + L);
                hb_bits_init(&b, row, 0);
                uint32_t n2;
                hb_region(&F, &b, nb, whole, at_end, ent, sink, &n2);
                __syncthreads();
                if (sink.sh) atomicOr((uint32_t *)(smem + sink.wd), sink.a);
                __syncthreads();
                // copy-out: whole 16-B blocks inside [beg, end), bytes at the edges
                uint8_t *gb = (uint8_t *)(ga - a0);
                const uint32_t beg = a0 + from, end = beg + keep, nq = (end + 15u) / 16u;
                for (uint32_t q = beg / 16u + tid; q < nq; q += blockDim.x) {
                    const uint32_t lo = 16u * q;
                    if (lo >= beg && lo + 16u <= end) {
                        *(u32x4 *)(gb + lo) = *(const u32x4 *)(stg + lo);
                    } else {
                        const uint32_t q0 = lo > beg ? lo : beg, q1 = lo + 16u < end ? lo + 16u : end;
                        for (uint32_t p = q0; p < q1; p++) gb[p] = stg[p];
                    }
                }
                got += keep;
            }
            base += tot;
            carry = carry_next;
            if (win && hb_window_done(base, skip, cap)) break;   // the window is full: no later round is loaded or walked
        }
        if (tid == 0) {
            res[idx].len = win ? got : base;
            res[idx].status = fail ? HH_ERR_INTERNAL
                              : win ? (got < cap ? HH_ERR_FORMAT : HH_OK) : base > cap ? HH_ERR_CAPACITY : HH_OK;
        }
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
void batch_setup(BatchDev *b, const FsmDev *fd, uint32_t G, uint32_t minlen) {
    b->ok = b->W = b->lds = b->grid_max = 0;
    b->G = G;
    b->minlen = minlen;
    if (!fd->ok) return;
    const uint32_t tabb = emf_tab_bytes(fd->ns, fd->K, fd->r);
    b->W = hb_pick_waves(tabb, fd->S, minlen, HB_LDS);
    if (!b->W || G % fd->K || G > fd->S) return;        // (no room for one tile's round beside the tables)
    b->lds = hb_lds_bytes(tabb, fd->S, minlen, b->W);
    b->ok = 1;
}

int batch_wait(BatchDev *b) {
    if (!b->pend) return HH_OK;
    b->pend = 0;
    FS_OK(hipEventSynchronize(b->end));
    return HH_OK;
}

void batch_free(BatchDev *b) {
    if (b->d_ws) (void)hipFree(b->d_ws);
    if (b->h_ws) (void)hipHostFree(b->h_ws);
    if (b->end) (void)hipEventDestroy(b->end);
    memset(b, 0, sizeof(*b));
}

// The workspace: need_d device bytes, need_h pinned host bytes (the device
// items' batch keeps nothing on the host).
int batch_ws(BatchDev *b, size_t need_d, size_t need_h) {
    if (b->d_size < need_d) {
        // (a synchronous call has returned, and a pending asynchronous decode
        // does not use this workspace; a batch of device items may still run)
        const int wrc = batch_wait(b);
        if (wrc != HH_OK) return wrc;
        if (b->d_ws) FS_OK(hipFree(b->d_ws));
        b->d_ws = nullptr;
        b->d_size = 0;
        const size_t sz = need_d + need_d / 8;
        if (hipMalloc(&b->d_ws, sz) != hipSuccess) return HH_ERR_NOMEM;
        b->d_size = sz;
    }
    if (b->h_size < need_h) {
        if (b->h_ws) FS_OK(hipHostFree(b->h_ws));
        b->h_ws = nullptr;
        b->h_size = 0;
        const size_t sz = need_h + need_h / 8;
        if (hipHostMalloc(&b->h_ws, sz, hipHostMallocDefault) != hipSuccess) {
            b->h_ws = nullptr;
            return HH_ERR_NOMEM;
        }
        b->h_size = sz;
    }
    return HH_OK;
}

// The resident workgroups of k_batch for the current tree, asked once.
static int batch_grid(BatchDev *b) {
    if (b->grid_max) return HH_OK;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)k_batch) != hipSuccess || fa.sharedSizeBytes != 0) return HH_ERR_INTERNAL;
    int per = 0, ncu = 0, dev = 0;
    FS_OK(hipGetDevice(&dev));
    FS_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_batch, (int)(64 * b->W), b->lds));
    FS_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (per < 1 || ncu < 1) return HH_ERR_UNSUPPORTED;
    b->grid_max = (uint32_t)(per * ncu);
    return HH_OK;
}

BatchGeo batch_geo(const BatchDev *b, const FsmDev *fd, uint64_t n) {
    BatchGeo geo;
    geo.ns = fd->ns; geo.K = fd->K; geo.r = fd->r; geo.S = fd->S; geo.G = b->G; geo.W = b->W;
    geo.pay_off = emf_tab_bytes(fd->ns, fd->K, fd->r);
    geo.misc_off = geo.pay_off + hb_pay_bytes(fd->S, b->W);
    geo.stg_off = (geo.misc_off + hb_misc_bytes() + 15u) & ~15u;
    geo.stg_bytes = hb_stage_bytes(fd->S, b->minlen, b->W);
    geo.n = (uint32_t)n;
    return geo;
}

int batch_decode(BatchDev *b, const FsmDev *fd, hipEvent_t *ev, const void *d_data, const hh_batch_item *items,
                 uint64_t n, void *d_out, uint64_t *out_len, int32_t *status, hipStream_t st, float *ms,
                 uint64_t *lanes) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    if (n > 0xffffffffull) return HH_ERR_UNSUPPORTED;
    const int grc = batch_grid(b);
    if (grc != HH_OK) return grc;
    const size_t dbytes = (size_t)n * sizeof(BatchDesc), rbytes = (size_t)n * sizeof(BatchRes);
    const int wrc = batch_ws(b, dbytes + rbytes, dbytes + rbytes);
    if (wrc != HH_OK) return wrc;
    BatchDesc *hd = (BatchDesc *)b->h_ws;
    BatchRes *hr = (BatchRes *)((uint8_t *)b->h_ws + dbytes);
    BatchDesc *dd = (BatchDesc *)b->d_ws;
    BatchRes *dr = (BatchRes *)((uint8_t *)b->d_ws + dbytes);
    // the longest streams first: the workgroups that take them start at once
    std::vector<uint32_t> ord((size_t)n);
    for (uint32_t i = 0; i < (uint32_t)n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return items[x].bits > items[y].bits; });
    uint64_t regions = 0;
    for (uint64_t k = 0; k < n; k++) {
        const hh_batch_item &s = items[ord[k]];
        hd[k] = BatchDesc{s.data_off, s.bits, s.out_off, s.cap, ord[k], 0, 0, 0};
        regions += (s.bits + fd->S - 1) / fd->S;
        hr[k].len = 0;
        hr[k].status = HB_UNTOUCHED;
    }
    *lanes = regions;
    const BatchGeo geo = batch_geo(b, fd, n);
    const FsmTab tab = {fd->ct, fd->b1, fd->tsym, fd->et, fd->er};
    // a batch of device items still running reads the workspace this one overwrites
    if (b->pend) FS_OK(hipStreamWaitEvent(st, b->end, 0));
    // descriptors and the untouched marks of the results, on the call's stream
    FS_OK(hipMemcpyAsync(dd, hd, dbytes + rbytes, hipMemcpyHostToDevice, st));
    const uint32_t grid = n < b->grid_max ? (uint32_t)n : b->grid_max;
    FS_OK(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_batch, dim3(grid), dim3(64 * b->W), b->lds, st, (const uint8_t *)d_data, dd, dr,
                       (uint8_t *)d_out, tab, geo);
    FS_OK(hipGetLastError());
    FS_OK(hipEventRecord(ev[1], st));
    FS_OK(hipMemcpyAsync(hr, dr, rbytes, hipMemcpyDeviceToHost, st));
    FS_OK(hipStreamSynchronize(st));
    b->pend = 0;                                          // (st waited for it, and is done)
    *ms = 0;
    (void)hipEventElapsedTime(ms, ev[0], ev[1]);
    int rc = HH_OK;
    for (uint64_t i = 0; i < n; i++) {
        const int s = hr[i].status == HB_UNTOUCHED ? HH_ERR_INTERNAL : (int)hr[i].status;
        out_len[i] = hr[i].len;
        if (status) status[i] = s;
        if (s != HH_OK && rc == HH_OK) rc = s;
    }
    return rc;
}

// Workspace of a batch of n device items: descriptors, results, the
// descriptors in index order (the plan's first kernel is the only one that
// reads the caller's list), a key byte per item, the plan's counters.
int batch_decode_items(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                       const hh_batch_item *d_items, uint64_t n, void *d_out, uint64_t out_bytes,
                       uint64_t *d_out_len, int32_t *d_status, hh_batch_summary *d_summary, hipStream_t st) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    if (n >= 0xffffffffull) return HH_ERR_UNSUPPORTED;    // (0xffffffff is the summary's "no stream")
    const int grc = batch_grid(b);
    if (grc != HH_OK) return grc;
    if (!b->end) FS_OK(hipEventCreateWithFlags(&b->end, hipEventDisableTiming));
    const size_t dbytes = (size_t)n * sizeof(BatchDesc), rbytes = (size_t)n * sizeof(BatchRes);
    const size_t kbytes = ((size_t)n + 255u) & ~(size_t)255u;
    const int wrc = batch_ws(b, 2 * dbytes + rbytes + kbytes + HB_PLAN_CTL_BYTES, 0);
    if (wrc != HH_OK) return wrc;
    uint8_t *w = (uint8_t *)b->d_ws;
    BatchDesc *dd = (BatchDesc *)w;
    BatchRes *dr = (BatchRes *)(w + dbytes);
    BatchDesc *tmp = (BatchDesc *)(w + dbytes + rbytes);
    uint8_t *key = w + 2 * dbytes + rbytes;
    uint32_t *ctl = (uint32_t *)(key + kbytes);
    // the batch before this one on another stream still uses the workspace
    // (on the same stream the order is the stream's)
    if (b->pend && b->pend_st != st) FS_OK(hipStreamWaitEvent(st, b->end, 0));
    const uint64_t RB = (uint64_t)HB_NR * b->W * fd->S;
    int rc = batch_plan_enqueue(d_items, (uint32_t)n, data_bytes, out_bytes, RB, dd, dr, tmp, key, ctl, d_summary, st);
    if (rc == HH_OK) {
        const BatchGeo geo = batch_geo(b, fd, n);
        const FsmTab tab = {fd->ct, fd->b1, fd->tsym, fd->et, fd->er};
        const uint32_t grid = n < b->grid_max ? (uint32_t)n : b->grid_max;
        hipLaunchKernelGGL(k_batch, dim3(grid), dim3(64 * b->W), b->lds, st, (const uint8_t *)d_data, dd, dr,
                           (uint8_t *)d_out, tab, geo);
        if (hipGetLastError() != hipSuccess) rc = HH_ERR_DEVICE;
    }
    if (rc == HH_OK) rc = batch_results_enqueue(dr, key, (uint32_t)n, d_out_len, d_status, d_summary, ctl, st);
    // (also after a failed launch: what was enqueued before it uses the workspace)
    FS_OK(hipEventRecord(b->end, st));
    b->pend = 1;
    b->pend_st = st;
    return rc;
}

// Range reads: the workspace and the grids are sized by the piece budget P,
// which the host knows; how many of the P slots hold a piece is device data.
// The slots past the pieces hold the empty descriptor (no round walked) and
// sort to the list's end (bin 0), so k_plan_place and k_batch run with n = P.
int batch_decode_read(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                      const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms, const hh_block_read *d_reads,
                      uint64_t m, uint32_t P, void *d_out, uint64_t out_bytes, uint64_t *d_read_len,
                      int32_t *d_status, hh_batch_summary *d_summary, hipStream_t st) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    const int grc = batch_grid(b);
    if (grc != HH_OK) return grc;
    if (!b->end) FS_OK(hipEventCreateWithFlags(&b->end, hipEventDisableTiming));
    const int wrc = batch_ws(b, read_ws_bytes(m, P), 0);
    if (wrc != HH_OK) return wrc;
    ReadWs w;
    read_ws_carve(&w, b->d_ws, m, P);
    if (b->pend && b->pend_st != st) FS_OK(hipStreamWaitEvent(st, b->end, 0));
    const uint64_t RB = (uint64_t)HB_NR * b->W * fd->S;
    int rc = read_plan_enqueue(&w, d_index, data_bytes, n_syms, block_syms, d_reads, (uint32_t)m, P, out_bytes, RB,
                               d_summary, st);
    if (rc == HH_OK) rc = batch_place_enqueue(w.tmp, w.key, P, w.ctl, w.desc, st);
    if (rc == HH_OK) {
        const BatchGeo geo = batch_geo(b, fd, P);
        const FsmTab tab = {fd->ct, fd->b1, fd->tsym, fd->et, fd->er};
        const uint32_t grid = P < b->grid_max ? P : b->grid_max;
        hipLaunchKernelGGL(k_batch, dim3(grid), dim3(64 * b->W), b->lds, st, (const uint8_t *)d_data,
                           (const BatchDesc *)w.desc, w.res, (uint8_t *)d_out, tab, geo);
        if (hipGetLastError() != hipSuccess) rc = HH_ERR_DEVICE;
    }
    if (rc == HH_OK) rc = read_results_enqueue(&w, (uint32_t)m, P, d_read_len, d_status, d_summary, st);
    // (also after a failed launch: what was enqueued before it uses the workspace)
    FS_OK(hipEventRecord(b->end, st));
    b->pend = 1;
    b->pend_st = st;
    return rc;
}
