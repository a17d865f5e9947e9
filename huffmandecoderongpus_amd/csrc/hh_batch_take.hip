// hh_batch_take.hip -- the record take (hh_decode_batch_take): m records of an
// index named by a device list of ids, decoded packed -- their bytes one after
// another in d_out, d_out_offs the offsets that delimit them -- with many
// records per round.  HIP (gfx950).  The rules are hh_batch_take_algo.h's.
//
// Launches, all on the caller's stream (a tile: HBT_TILE records):
//   k_take_len    a thread per taken record: the only kernel that reads d_ids
//                 and d_index.  The id and the row checked, rec[j] = the row's
//                 data_off, bits and the record's length (0, 0, 0 for a bad
//                 one, whose offsets never become addresses), d_status[j] =
//                 HH_OK or HH_ERR_ARG for now, the tile's length.
//   k_take_top    one workgroup: the tiles' lengths into their exclusive
//                 saturating sums, HBT_TILE tiles a step.
//   k_take_offs   a thread per record: d_out_offs, the record's fate
//                 (hbt_fate: its final status, or HH_ERR_INTERNAL until k_take
//                 reaches the stream), its regions; the tile's streams and
//                 regions.
//   k_take_top    those two into exclusive sums; the totals: streams, slots.
//   k_take_fill   a thread per record: a stream's descriptor at its place in
//                 take order, its first slot.
//   k_take_cut    a thread per share edge: the workgroups' first streams.
//   k_take        the packed rounds (below).
//   k_take_results  a thread per record: the summary, k_batch_results' way.
// No workgroup steps through the records: k_take_top steps through their tile
// sums, 2^20 records a step.
//
// k_take: workgroup b decodes the streams cut[b] .. cut[b + 1] in rounds of
// 64 W slots numbered from its first stream's first slot.  Per round: thread
// t looks at stream next + t and, when it starts in the round, leaves its
// mark and its data_off and bits in LDS by ordinal (it is the stream's OWNER
// for the round: it knows the length and the output offset and settles the
// stream after the scan); a maximum scan over the marks gives every lane its
// stream and region; the lane loads its region's words (bounded by
// data_bytes), and guess, count, fix rounds, scan and emission into the
// staging are k_batch's.  The owners compare each stream's count with its
// length; where all agree the staging is one range of d_out and goes out as
// k_batch's (whole 16-byte blocks strictly inside, bytes at the edges), else
// every lane copies its own region's bytes, clipped to its record.  The
// stream of the round's last lane, when it goes on, is carried into the next
// round (state, regions walked, symbols so far) through the round's record in
// LDS.
//
// LDS (dynamic only, from address 0): k_batch's -- tables, payload rows, wx /
// wt / chg -- then the round's record, the marks, a stream's first byte in the
// round by ordinal, then the staging, which holds data_off and bits by
// ordinal from the round's start until the payload is loaded (the staging is
// written by the emission and read by the copy-out only).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include "hh_batch.h"
#include "hh_batch_algo.h"
#include "hh_batch_take_algo.h"
#include "hh_fsm_kern.h"

#define HBT_TB HBT_TILE
static_assert(sizeof(hbt_desc) == 48 && sizeof(hh_batch_item) == 32, "layouts the kernels assume");
static_assert(64u * HB_WMAX <= (1u << HBT_POS_BITS), "a mark holds a round's slot");

struct TakeRec {
    uint64_t data_off, bits, len;
};
// ctl (u64 words): the streams, the slots, the sum of the lengths, the results' workgroups finished (u32)
#define HBT_CTL_NS 0u
#define HBT_CTL_SLOTS 1u
#define HBT_CTL_LEN 2u
#define HBT_CTL_DONE 3u
#define HBT_CTL_BYTES 64u

struct TakeGeo {
    BatchGeo g;
    uint32_t tm_off, sdo_off, sdb_off, mk_off, hd_off;    // LDS byte offsets
};
// the round's record (tm): u64 words, then u32 words
#define TM_GA 0u
#define TM_DOFF 1u
#define TM_BITS 2u
#define TM_LEN 3u
#define TM_OUT 4u
#define TM_J 5u
#define TM_Q 6u
#define TM_CNT 7u
#define TM32_BAD 16u
#define TM32_CHAS 17u
#define TM32_WM 20u
static_assert((TM32_WM + HB_WMAX) * 4u <= HBT_MISC_BYTES, "the round's record fits");

// One tile of HBT_TB values: this thread's exclusive prefix within the
// workgroup, *tot the tile's sum; saturating.
__device__ __forceinline__ uint64_t take_scan_tile(uint64_t v, uint64_t *s_w, uint64_t *tot) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x = hbt_sat_add(x, y);
    }
    if (lane == 63) s_w[wv] = x;
    uint64_t ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = 0;
    __syncthreads();
    uint64_t base = 0, t = 0;
    for (uint32_t i = 0; i < HBT_TB / 64; i++) {
        base = i < wv ? hbt_sat_add(base, s_w[i]) : base;
        t = hbt_sat_add(t, s_w[i]);
    }
    __syncthreads();
    *tot = t;
    return hbt_sat_add(base, ex);
}

__global__ __launch_bounds__(HBT_TB) void k_take_len(const uint64_t *__restrict__ ids,
                                                     const hh_batch_item *__restrict__ index, uint64_t nrec, uint32_t m,
                                                     uint64_t data_bytes, TakeRec *__restrict__ rec,
                                                     int32_t *__restrict__ status, uint64_t *__restrict__ tl,
                                                     hh_batch_summary *__restrict__ sum) {
    __shared__ uint64_t s_w[HBT_TB / 64];
    const uint32_t j = blockIdx.x * HBT_TB + threadIdx.x;
    uint64_t len = 0;
    if (j < m) {
        const uint64_t r = ids ? ids[j] : j;
        TakeRec t = {0, 0, 0};
        int ok = 0;
        if (r < nrec) {
            const hh_batch_item it = index[r];
            ok = hbt_row_ok(r, nrec, it.data_off, it.bits, data_bytes);
            if (ok) t = TakeRec{it.data_off, it.bits, it.cap};
        }
        rec[j] = t;
        status[j] = ok ? HH_OK : HH_ERR_ARG;
        len = t.len;
    }
    uint64_t tot;
    (void)take_scan_tile(len, s_w, &tot);
    if (threadIdx.x == 0) tl[blockIdx.x] = tot;
    if (j == 0 && sum) *sum = hh_batch_summary{0, 0, 0xffffffffu, HH_OK, 0};
}

// One workgroup: nt tile sums into exclusive ones in place, HBT_TB a step with
// the carry; *ta their sum.  The same for b when given.
__global__ __launch_bounds__(HBT_TB) void k_take_top(uint64_t *__restrict__ a, uint64_t *__restrict__ b, uint32_t nt,
                                                     uint64_t *__restrict__ ta, uint64_t *__restrict__ tb) {
    __shared__ uint64_t s_w[HBT_TB / 64];
    uint64_t ca = 0, cb = 0, tot;
    for (uint32_t t0 = 0; t0 < nt; t0 += HBT_TB) {
        const uint32_t t = t0 + threadIdx.x;
        const uint64_t xa = take_scan_tile(t < nt ? a[t] : 0, s_w, &tot);
        if (t < nt) a[t] = hbt_sat_add(ca, xa);
        ca = hbt_sat_add(ca, tot);
        if (b) {
            const uint64_t xb = take_scan_tile(t < nt ? b[t] : 0, s_w, &tot);
            if (t < nt) b[t] = hbt_sat_add(cb, xb);
            cb = hbt_sat_add(cb, tot);
        }
    }
    if (threadIdx.x == 0) {
        *ta = ca;
        if (b) *tb = cb;
    }
}

__global__ __launch_bounds__(HBT_TB) void k_take_offs(const TakeRec *__restrict__ rec, uint32_t m,
                                                      const uint64_t *__restrict__ tl, uint64_t out_bytes, uint32_t S,
                                                      uint64_t *__restrict__ out_offs, int32_t *__restrict__ status,
                                                      uint64_t *__restrict__ reg, uint64_t *__restrict__ tf,
                                                      uint64_t *__restrict__ tr) {
    __shared__ uint64_t s_w[HBT_TB / 64];
    const uint32_t j = blockIdx.x * HBT_TB + threadIdx.x;
    TakeRec t = {0, 0, 0};
    if (j < m) t = rec[j];
    uint64_t tot;
    const uint64_t off = hbt_sat_add(tl[blockIdx.x], take_scan_tile(t.len, s_w, &tot));
    uint64_t regions = 0;
    if (j < m) {
        const uint64_t end = hbt_sat_add(off, t.len);
        out_offs[j] = off;
        if (j == m - 1u) out_offs[m] = end;
        const int32_t f = hbt_fate(status[j] == HH_OK, t.bits, t.len, end, out_bytes);
        status[j] = f == HBT_STREAM ? HH_ERR_INTERNAL : f;
        regions = f == HBT_STREAM ? hbt_regions(t.bits, S) : 0u;
        reg[j] = regions;
    }
    (void)take_scan_tile(regions != 0, s_w, &tot);
    if (threadIdx.x == 0) tf[blockIdx.x] = tot;
    (void)take_scan_tile(regions, s_w, &tot);
    if (threadIdx.x == 0) tr[blockIdx.x] = tot;
}

__global__ __launch_bounds__(HBT_TB) void k_take_fill(const TakeRec *__restrict__ rec, const uint64_t *__restrict__ reg,
                                                      const uint64_t *__restrict__ out_offs, uint32_t m,
                                                      const uint64_t *__restrict__ tf, const uint64_t *__restrict__ tr,
                                                      hbt_desc *__restrict__ desc) {
    __shared__ uint64_t s_w[HBT_TB / 64];
    const uint32_t j = blockIdx.x * HBT_TB + threadIdx.x;
    const uint64_t regions = j < m ? reg[j] : 0u;
    uint64_t tot;
    const uint64_t at = tf[blockIdx.x] + take_scan_tile(regions != 0, s_w, &tot);
    const uint64_t slot0 = hbt_sat_add(tr[blockIdx.x], take_scan_tile(regions, s_w, &tot));
    if (regions && at < m) {                              // (always: the streams are among the m records)
        const TakeRec t = rec[j];
        desc[at] = hbt_desc{t.data_off, t.bits, slot0, out_offs[j], t.len, j};
    }
}

// A thread per share edge: cut[e], workgroup e's first stream; cut[grid] = the
// streams.  Slots that do not fit 64 bits (never: a slot is 32 bits of a
// payload or more) leave every workgroup without a stream.
__global__ __launch_bounds__(256) void k_take_cut(const hbt_desc *__restrict__ desc, const uint64_t *__restrict__ ctl,
                                                  uint32_t grid, uint32_t NL, uint32_t *__restrict__ cut) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e > grid) return;
    const uint64_t nslots = ctl[HBT_CTL_SLOTS];
    const uint32_t ns = nslots == ~0ull ? 0u : (uint32_t)ctl[HBT_CTL_NS];
    cut[e] = e == grid ? ns : hbt_edge(desc, ns, nslots, hbt_share(nslots, grid, NL, 0u), e);
}

__global__ __launch_bounds__(64 * HB_WMAX) void k_take(const uint8_t *__restrict__ data, uint64_t data_bytes,
                                                       const hbt_desc *__restrict__ desc,
                                                       const uint32_t *__restrict__ cut, uint8_t *__restrict__ out,
                                                       int32_t *__restrict__ status, FsmTab tab, TakeGeo tg) {
    extern __shared__ __align__(16) uint8_t smem[];
    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cut[blockIdx.x]);
    const uint32_t s1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cut[blockIdx.x + 1]);
    if (s0 >= s1) return;                                 // (an empty share: before the tables are loaded)
    const BatchGeo &geo = tg.g;
    const uint32_t ns = geo.ns, K = geo.K, r = geo.r, S = geo.S, G = geo.G, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t W = geo.W, SW = S / 32u, RW = hb_row_words(S), NL = HB_NR * W;
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
    uint64_t *tm = (uint64_t *)(smem + tg.tm_off), *sdo = (uint64_t *)(smem + tg.sdo_off);
    uint64_t *sdb = (uint64_t *)(smem + tg.sdb_off);
    uint32_t *tm32 = (uint32_t *)tm, *mk = (uint32_t *)(smem + tg.mk_off), *hd = (uint32_t *)(smem + tg.hd_off);
    const bool lds0 = lds_base_is_zero(smem);
    const uint32_t jr = tid;                              // the lane's slot of a round (blockDim.x == NL)
    const uint32_t *g32 = (const uint32_t *)data;
    mk[jr] = 0;
    const uint64_t base0 = uni64(desc[s0].slot0);         // the workgroup numbers slots from its first stream
    uint32_t nxt = s0;                                    // the first stream that has not started
    // the stream carried into the round: its row, the regions walked, the symbols so far, the state
    uint32_t c_has = 0, carry = 0, fail = lds0 ? 0u : 1u;
    uint64_t c_doff = 0, c_bits = 0, c_len = 0, c_out = 0, c_j = 0, c_q = 0, c_cnt = 0;

    for (uint64_t lo = 0; (c_has || nxt < s1) && !fail; lo += NL) {
        __syncthreads();                                  // the round before is done with the rows, the staging and the record
        // the streams that start in the round: thread t owns stream nxt + t
        hbt_desc od = {0, 0, 0, 0, 0, 0};
        bool own = false;
        uint32_t spos = 0;
        if ((uint64_t)nxt + tid < s1) {
            od = desc[nxt + tid];
            const uint64_t sl = od.slot0 - base0;
            if (sl >= lo && sl - lo < NL) {
                own = true;
                spos = (uint32_t)(sl - lo);
                mk[spos] = hbt_mark(tid + 1u, spos);
                sdo[tid + 1u] = od.data_off;
                sdb[tid + 1u] = od.bits;
            }
        }
        if (tid == 0) {
            tm32[TM32_BAD] = 0;
            tm32[TM32_CHAS] = 0;
            tm[TM_GA] = c_has ? c_out + c_cnt : od.out_off;   // the output offset of the round's byte 0
        }
        __syncthreads();
        uint32_t mv = mk[jr];
        mk[jr] = 0;                                       // (for the next round)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)mv, o, 64);
            if (lane >= (uint32_t)o) mv = mv > y ? mv : y;
        }
        if (lane == 63u) tm32[TM32_WM + wv] = mv;
        __syncthreads();
        uint32_t mlast = 0;
        for (uint32_t v = 0; v < W; v++) {
            const uint32_t t = tm32[TM32_WM + v];
            mv = v < wv && t > mv ? t : mv;
            mlast = t > mlast ? t : mlast;
        }
        const uint32_t o_last = hbt_mark_ord(mlast), o = hbt_mark_ord(mv);
        const uint64_t ga = tm[TM_GA];
        if (!o_last && !c_has) fail = 1u;                 // (cannot happen: the slots are the streams' regions)
        const uint64_t q = hbt_region_of(jr, mv, c_q);
        const uint64_t doff = o ? sdo[o] : c_doff, bits = o || c_has ? (o ? sdb[o] : c_bits) : 0u;
        int whole, at_end;
        const uint32_t nb = hb_span(q * S, S, bits, &whole, &at_end);
        // the lane's region of its own stream; what lies past data_bytes reads as 0
        uint32_t *row = pay + jr * RW;
        if (nb) {
            const uint64_t w0 = doff / 4u + q * SW;
#pragma unroll 4
            for (uint32_t k = 0; k < SW; k++) row[k] = (w0 + k) * 4u + 4u <= data_bytes ? g32[w0 + k] : 0u;
        }
        if (tid == 0) chg[0] = 0;
        __syncthreads();
        const int exact = hbt_exact(jr, q);
        hb_bits b;
        uint32_t ent = exact ? hbt_entry(q, carry) : 0u, x, n;
        if (!exact && G && nb) {
            hb_bits_init(&b, pay + (jr - 1u) * RW, S - G);
            ent = hb_guess(&F, &b, G);
        }
        hb_no_sink none;
        hb_bits_init(&b, row, 0);
        x = hb_region(&F, &b, nb, whole, at_end, ent, none, &n);
        uint32_t c3 = 0, fr = 0;
        for (;; fr++) {
            if (lane == 63u) wx[wv] = x;
            const uint32_t c3n = c3 == 2u ? 0u : c3 + 1u;
            if (tid == 0) chg[c3n] = 0;
            __syncthreads();
            uint32_t pred = shfl_up1(x);
            if (lane == 0) pred = wv ? wx[wv - 1u] : carry;
            const int again = hbt_fix(exact, nb, pred, &ent);
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
        const uint32_t carry_next = wx[W - 1u];
        // one scan over all slots
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
        if (jr == 0 || q == 0) hd[o] = L;                 // a stream's first byte in the round
        if (jr == NL - 1u) hd[o + 1u] = tot;              // (the last stream's end)
        const uint32_t a0 = (uint32_t)(((uintptr_t)out + ga) & 15u);
        if (a0 + tot + 8u > geo.stg_bytes) fail = 1u;     // (the host sized it for the most a round holds)
        if (fail) break;                                  // (uniform; the streams not settled stay HH_ERR_INTERNAL)
        if (tid == 0) *(uint32_t *)(stg + ((a0 + tot) & ~3u)) = 0u;   // the last, partial dword: ORs only
        BatchSink sink;
        sink.init(smem, geo.stg_off + a0 + L);
        hb_bits_init(&b, row, 0);
        uint32_t n2;
        hb_region(&F, &b, nb, whole, at_end, ent, sink, &n2);
        __syncthreads();
        if (sink.sh) atomicOr((uint32_t *)(smem + sink.wd), sink.a);
        // the owners settle their streams: the one that goes on leaves the next round's record
        if (own) {
            const uint32_t first = hd[tid + 1u], nr = hd[tid + 2u] - first;
            const int ended = spos + hbt_regions(od.bits, S) <= NL;
            int32_t st;
            if (hbt_settle(0u, nr, od.len, ended, &st) || !hbt_in_place(ga, first, od.out_off)) tm32[TM32_BAD] = 1u;
            if (ended) {
                status[od.j] = st;
            } else {
                tm[TM_DOFF] = od.data_off; tm[TM_BITS] = od.bits; tm[TM_LEN] = od.len; tm[TM_OUT] = od.out_off;
                tm[TM_J] = od.j; tm[TM_Q] = NL - spos; tm[TM_CNT] = nr;
                tm32[TM32_CHAS] = 1u;
            }
        }
        if (tid == 0 && c_has) {
            const uint32_t nr = hd[1] - hd[0];
            const int ended = hbt_regions(c_bits, S) - c_q <= NL;
            int32_t st;
            if (hbt_settle(c_cnt, nr, c_len, ended, &st)) tm32[TM32_BAD] = 1u;
            if (ended) {
                status[c_j] = st;
            } else {
                tm[TM_DOFF] = c_doff; tm[TM_BITS] = c_bits; tm[TM_LEN] = c_len; tm[TM_OUT] = c_out;
                tm[TM_J] = c_j; tm[TM_Q] = c_q + NL; tm[TM_CNT] = c_cnt + nr;
                tm32[TM32_CHAS] = 1u;
            }
        }
        __syncthreads();
        if (!tm32[TM32_BAD]) {
            // every stream has its length: the round is one range of the output.
            // copy-out: whole 16-B blocks inside [beg, end), bytes at the edges
            uint8_t *gb = out + ga - a0;
            const uint32_t beg = a0, end = a0 + tot, nq = (end + 15u) / 16u;
            for (uint32_t p16 = beg / 16u + tid; p16 < nq; p16 += blockDim.x) {
                const uint32_t l16 = 16u * p16;
                if (l16 >= beg && l16 + 16u <= end) {
                    *(u32x4 *)(gb + l16) = *(const u32x4 *)(stg + l16);
                } else {
                    const uint32_t q0 = l16 > beg ? l16 : beg, q1 = l16 + 16u < end ? l16 + 16u : end;
                    for (uint32_t p = q0; p < q1; p++) gb[p] = stg[p];
                }
            }
        } else if (n) {
            // index and data disagree somewhere in the round: every lane its own bytes, clipped to its record
            uint64_t s_out = c_out, s_len = c_len;
            if (o) {
                s_out = desc[nxt + o - 1u].out_off;
                s_len = desc[nxt + o - 1u].len;
            }
            const uint64_t pos = (o ? 0u : c_cnt) + (L - hd[o]);
            const uint32_t keep = hb_clip(pos, n, s_len);
            uint8_t *dst = out + s_out + pos;
            const uint8_t *src = stg + a0 + L;
            for (uint32_t p = 0; p < keep; p++) dst[p] = src[p];
        }
        // the next round's carried stream
        c_has = (uint32_t)__builtin_amdgcn_readfirstlane((int)tm32[TM32_CHAS]);
        if (c_has) {
            c_doff = uni64(tm[TM_DOFF]); c_bits = uni64(tm[TM_BITS]); c_len = uni64(tm[TM_LEN]);
            c_out = uni64(tm[TM_OUT]); c_j = uni64(tm[TM_J]); c_q = uni64(tm[TM_Q]); c_cnt = uni64(tm[TM_CNT]);
        }
        nxt += o_last;
        carry = carry_next;
    }
}

// A thread per taken record: the summary.  total_len: the lengths of the
// HH_OK records; the last workgroup to finish fills first_status.
__global__ __launch_bounds__(256) void k_take_results(const uint64_t *__restrict__ out_offs,
                                                      const int32_t *__restrict__ status, uint32_t m,
                                                      hh_batch_summary *sum, uint32_t *done) {
    __shared__ uint64_t s_len[4];
    __shared__ uint32_t s_bad[4], s_first[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, i = blockIdx.x * 256u + tid;
    uint64_t len = 0;
    uint32_t bad = 0, first = 0xffffffffu;
    if (i < m) {
        if (status[i] == HH_OK) {
            len = out_offs[i + 1] - out_offs[i];
        } else {
            bad = 1;
            first = i;
        }
    }
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
    for (uint32_t v = 1; v < 4u; v++) {
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
    if (atomicAdd(done, 1u) != gridDim.x - 1u) return;
    __threadfence();
    const uint32_t ff = atomicMin(&sum->first_failed, 0xffffffffu);   // (an atomic read)
    if (ff < m) sum->first_status = status[ff];
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// k_take's shape for the decoder's tree: W of its own (the marks take LDS
// that k_batch does not need), the resident workgroups asked once per shape.
static int take_shape(BatchDev *b, const FsmDev *fd, uint32_t *W, uint32_t *lds) {
    const uint32_t tabb = emf_tab_bytes(fd->ns, fd->K, fd->r);
    *W = hbt_pick_waves(tabb, fd->S, b->minlen, HB_LDS);
    if (!*W) return HH_ERR_UNSUPPORTED;
    *lds = hbt_lds_bytes(tabb, fd->S, b->minlen, *W);
    if (b->tk_grid && b->tk_W == *W && b->tk_lds == *lds) return HH_OK;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)k_take) != hipSuccess || fa.sharedSizeBytes != 0) return HH_ERR_INTERNAL;
    int per = 0, ncu = 0, dev = 0;
    FS_OK(hipGetDevice(&dev));
    FS_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_take, (int)(64 * *W), *lds));
    FS_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (per < 1 || ncu < 1) return HH_ERR_UNSUPPORTED;
    b->tk_grid = (uint32_t)(per * ncu);
    b->tk_W = *W;
    b->tk_lds = *lds;
    return HH_OK;
}

int batch_take_waves(const BatchDev *b, const FsmDev *fd, uint32_t *W, uint32_t *lds) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    const uint32_t tabb = emf_tab_bytes(fd->ns, fd->K, fd->r);
    *W = hbt_pick_waves(tabb, fd->S, b->minlen, HB_LDS);
    if (!*W) return HH_ERR_UNSUPPORTED;
    *lds = hbt_lds_bytes(tabb, fd->S, b->minlen, *W);
    return HH_OK;
}

int batch_decode_take(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                      const hh_batch_item *d_index, uint64_t nrec, const uint64_t *d_ids, uint64_t m, void *d_out,
                      uint64_t out_bytes, uint64_t *d_out_offs, int32_t *d_status, hh_batch_summary *d_summary,
                      hipStream_t st) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    if (m >= 0xffffffffull || nrec >= 0xffffffffull) return HH_ERR_UNSUPPORTED;
    uint32_t W = 0, lds = 0;
    const int src = take_shape(b, fd, &W, &lds);
    if (src != HH_OK) return src;
    if (!b->end) FS_OK(hipEventCreateWithFlags(&b->end, hipEventDisableTiming));
    const uint32_t m32 = (uint32_t)m, nt = (m32 + HBT_TB - 1u) / HBT_TB, NL = HB_NR * W;
    const uint32_t grid = m32 < b->tk_grid ? m32 : b->tk_grid;
    // workspace per record: its row (24), its regions (8), its descriptor (48); per tile three sums
    const size_t o_rec = 0, o_reg = o_rec + al256((size_t)m * sizeof(TakeRec)), o_desc = o_reg + al256((size_t)m * 8),
                 o_tl = o_desc + al256((size_t)m * sizeof(hbt_desc)), o_tf = o_tl + al256((size_t)nt * 8),
                 o_tr = o_tf + al256((size_t)nt * 8), o_cut = o_tr + al256((size_t)nt * 8),
                 o_ctl = o_cut + al256(((size_t)grid + 1) * 4), need = o_ctl + HBT_CTL_BYTES;
    const int wrc = batch_ws(b, need, 0);
    if (wrc != HH_OK) return wrc;
    uint8_t *w = (uint8_t *)b->d_ws;
    TakeRec *rec = (TakeRec *)(w + o_rec);
    uint64_t *reg = (uint64_t *)(w + o_reg), *tl = (uint64_t *)(w + o_tl), *tf = (uint64_t *)(w + o_tf),
             *tr = (uint64_t *)(w + o_tr), *ctl = (uint64_t *)(w + o_ctl);
    hbt_desc *desc = (hbt_desc *)(w + o_desc);
    uint32_t *cut = (uint32_t *)(w + o_cut);
    // the batch before this one on another stream still uses the workspace
    if (b->pend && b->pend_st != st) FS_OK(hipStreamWaitEvent(st, b->end, 0));
    int rc = HH_OK;
    do {
        rc = HH_ERR_DEVICE;
        if (hipMemsetAsync(ctl, 0, HBT_CTL_BYTES, st) != hipSuccess) break;
        hipLaunchKernelGGL(k_take_len, dim3(nt), dim3(HBT_TB), 0, st, d_ids, d_index, nrec, m32, data_bytes, rec,
                           d_status, tl, d_summary);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_take_top, dim3(1), dim3(HBT_TB), 0, st, tl, (uint64_t *)nullptr, nt, ctl + HBT_CTL_LEN,
                           (uint64_t *)nullptr);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_take_offs, dim3(nt), dim3(HBT_TB), 0, st, rec, m32, tl, out_bytes, fd->S, d_out_offs,
                           d_status, reg, tf, tr);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_take_top, dim3(1), dim3(HBT_TB), 0, st, tf, tr, nt, ctl + HBT_CTL_NS, ctl + HBT_CTL_SLOTS);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_take_fill, dim3(nt), dim3(HBT_TB), 0, st, rec, reg, d_out_offs, m32, tf, tr, desc);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_take_cut, dim3(grid / 256u + 1u), dim3(256), 0, st, desc, ctl, grid, NL, cut);
        if (hipGetLastError() != hipSuccess) break;
        TakeGeo tg;
        tg.g.ns = fd->ns; tg.g.K = fd->K; tg.g.r = fd->r; tg.g.S = fd->S; tg.g.G = b->G; tg.g.W = W;
        tg.g.pay_off = emf_tab_bytes(fd->ns, fd->K, fd->r);
        tg.g.misc_off = tg.g.pay_off + hb_pay_bytes(fd->S, W);
        tg.tm_off = (tg.g.misc_off + hb_misc_bytes() + 15u) & ~15u;
        tg.mk_off = tg.tm_off + HBT_MISC_BYTES;
        tg.hd_off = tg.mk_off + NL * 4u;
        tg.g.stg_off = tg.tm_off + hbt_extra_bytes(W);
        tg.g.stg_bytes = hb_stage_bytes(fd->S, b->minlen, W);
        tg.sdo_off = tg.g.stg_off;                         // (in the staging, free until the emission)
        tg.sdb_off = tg.sdo_off + (NL + 1u) * 8u;
        tg.g.n = m32;
        if (tg.hd_off + (NL + 2u) * 4u > tg.g.stg_off || tg.sdb_off + (NL + 1u) * 8u > lds ||
            tg.g.stg_off + tg.g.stg_bytes > lds) { rc = HH_ERR_INTERNAL; break; }
        const FsmTab tab = {fd->ct, fd->b1, fd->tsym, fd->et, fd->er};
        hipLaunchKernelGGL(k_take, dim3(grid), dim3(64 * W), lds, st, (const uint8_t *)d_data, data_bytes,
                           (const hbt_desc *)desc, (const uint32_t *)cut, (uint8_t *)d_out, d_status, tab, tg);
        if (hipGetLastError() != hipSuccess) break;
        if (d_summary) {
            hipLaunchKernelGGL(k_take_results, dim3((m32 + 255u) / 256u), dim3(256), 0, st,
                               (const uint64_t *)d_out_offs, (const int32_t *)d_status, m32, d_summary,
                               (uint32_t *)(ctl + HBT_CTL_DONE));
            if (hipGetLastError() != hipSuccess) break;
        }
        rc = HH_OK;
    } while (0);
    // (also after a failed launch: what was enqueued before it uses the workspace)
    FS_OK(hipEventRecord(b->end, st));
    b->pend = 1;
    b->pend_st = st;
    return rc;
}
