// hh_batch_gather.hip -- gathered range reads over a block-coded buffer
// (hh_decode_blocks_gather): the reads of hh_decode_blocks_read, but every
// touched block is walked once for all the pieces that fall into it, where
// k_batch walks it once per piece.  HIP (gfx950).  The rules are
// hh_batch_read_algo.h's (reads -> pieces) and hh_batch_gather_algo.h's
// (pieces -> blocks, the walk's end, a piece's result, the copy's split).
//
// The host knows m, the piece budget P and the blocks nb; how many slots hold
// a piece and how many blocks are touched is device data (ctl's TOTAL, WALKS).
//
//   (memset)         ctl; per block the end, the count, the placement cursor
//   k_read_count, k_read_scan   hh_batch_read.hip's, as they are
//   k_gather_fill    a thread per slot below the total: owner, window and the
//                    block's index entry as k_read_fill; the piece record by
//                    slot, own[s], res[s] untouched, the key byte (the invalid
//                    mark for a bad entry, so k_read_gather serves unchanged);
//                    a valid piece adds 1 to its block's count and folds skip
//                    + cap into the block's end (atomic max)
//   k_gather_sums    a workgroup per 1024 blocks: the pieces and the touched
//                    blocks of its tile
//   k_gather_top     one workgroup: those sums into exclusive ones, 1024 at a
//                    step with the carry; the touched blocks T into ctl
//   k_gather_first   a workgroup per 1024 blocks again: a block's first list
//                    position = its tile's sum + the scan inside the tile;
//                    the touched blocks per bin (hbp_bin of the block's bits)
//   k_gather_place   a thread per slot: first[block] + an atomic add on the
//                    block's cursor -> the piece's place in the list
//   k_gather_walks   a thread per block: a touched block's walk descriptor to
//                    its bin's place, longest first (k_plan_place's scheme)
//   k_gather         the walk, below
//   k_read_gather, k_read_results   hh_batch_read.hip's, as they are
//
// k_gather: a workgroup of W waves takes walks blockIdx.x, + gridDim.x, ...
// below T.  A round is k_batch's up to the scan (same hb_* functions, same
// LDS layout, BatchGeo); then the threads stride over the block's piece list:
// when no piece has bytes in the round it is counted only, else it is emitted
// once into the staging from offset 0 and every piece that has bytes in it
// copies them out.  Copy-out: the list goes through the waves 64 pieces at a
// time, a lane per piece.  A part of at most HBG_SMALL bytes is stored byte by
// byte by its lane (the chunks dealt to the waves in turn); a longer part is
// taken by the whole workgroup, the lanes across its 16-byte blocks
// (hbg_copy_split: whole blocks only where the destination is aligned and all
// 16 bytes are the piece's, single bytes at the edges).  The staging offset of
// such a block has any alignment, so its value is built from five aligned
// dwords.  The walk ends with the round that reaches the block's end; then
// every piece's result is written once from the symbols seen.
// All atomics are ordinary vector atomics on device memory.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <mutex>

#include "hh_batch.h"
#include "hh_batch_algo.h"
#include "hh_batch_gather_algo.h"
#include "hh_batch_plan_algo.h"
#include "hh_batch_read_algo.h"
#include "hh_fsm_kern.h"

#define HBG_TB 256u                  // threads per workgroup of the per-slot and per-block kernels
#define HBG_SCAN_TB 1024u            // blocks per workgroup of the scan
#define HBG_NOBLK 0xffffffffu        // a piece whose index entry broke a rule

// a piece by slot and in its block's list; a walk
struct GatherPiece {
    uint64_t skip, cap, out_off;
    uint32_t slot, blk;
};
struct GatherWalk {
    uint64_t data_off, bits, end;
    uint32_t first, cnt;
};
static_assert(sizeof(GatherPiece) == 32 && sizeof(GatherWalk) == 32 && sizeof(GatherPiece) <= sizeof(BatchDesc),
              "a piece record fits a descriptor's place in the workspace");
static_assert((HB_CTL_WALKS + 1u) * 4u <= HB_PLAN_CTL_BYTES && HB_CTL_WALKS >= HB_CTL_FIRST + 2u, "ctl's words");

__global__ __launch_bounds__(HBG_TB) void k_gather_fill(uint32_t P, const uint64_t *__restrict__ start, uint32_t m,
                                                        const hh_block_read *__restrict__ copy,
                                                        const hh_batch_item *__restrict__ index, uint64_t data_bytes,
                                                        uint64_t B, GatherPiece *__restrict__ pc,
                                                        uint8_t *__restrict__ key, BatchRes *__restrict__ res,
                                                        uint32_t *__restrict__ own, const uint32_t *__restrict__ ctl,
                                                        uint32_t *bcnt, uint64_t *bend) {
    const uint32_t s = blockIdx.x * HBG_TB + threadIdx.x;
    if (s >= P || s >= ctl[HB_CTL_TOTAL]) return;         // (final: k_read_scan is done)
    const uint64_t i = hbr_owner(start, m, s);
    const hh_block_read r = copy[i];
    uint64_t blk, skip, cap, out_off;
    hbr_piece(r.src_off, r.len, r.dst_off, B, s - start[i], &blk, &skip, &cap, &out_off);
    const uint64_t data_off = index[blk].data_off, bits = index[blk].bits;
    // an entry that breaks a rule never becomes an address
    const bool ok = hbp_item_ok(data_off, bits, 0, 0, data_bytes, 0) != 0;
    pc[s] = ok ? GatherPiece{skip, cap, out_off, s, (uint32_t)blk} : GatherPiece{0, 0, 0, s, HBG_NOBLK};
    key[s] = (uint8_t)(ok ? 0u : HBP_INVALID);
    own[s] = (uint32_t)i;
    res[s] = BatchRes{0, HB_UNTOUCHED};
    if (ok) {
        atomicAdd(&bcnt[blk], 1u);
        atomicMax((unsigned long long *)&bend[blk], (unsigned long long)hbg_piece_end(skip, cap));
    }
}

// The pieces and the touched blocks of a tile of HBG_SCAN_TB blocks: the
// workgroup's inclusive scan of both (x, y), the totals in *tx, *ty.
__device__ __forceinline__ void tile_scan(uint32_t *x, uint32_t *y, uint32_t *tx, uint32_t *ty, uint32_t *s_x,
                                          uint32_t *s_y) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t ix = (uint32_t)wave_incl_scan((int32_t)*x), iy = (uint32_t)wave_incl_scan((int32_t)*y);
    if (lane == 63u) {
        s_x[wv] = ix;
        s_y[wv] = iy;
    }
    __syncthreads();
    uint32_t ox = 0, oy = 0, sx = 0, sy = 0;
    for (uint32_t v = 0; v < HBG_SCAN_TB / 64u; v++) {
        const uint32_t a = s_x[v], b = s_y[v];
        ox += v < wv ? a : 0u;
        oy += v < wv ? b : 0u;
        sx += a;
        sy += b;
    }
    __syncthreads();                                      // (s_x, s_y may be written again)
    *x = ox + ix;
    *y = oy + iy;
    *tx = sx;
    *ty = sy;
}

__global__ __launch_bounds__(HBG_SCAN_TB) void k_gather_sums(const uint32_t *__restrict__ bcnt, uint32_t nb,
                                                             uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_x[HBG_SCAN_TB / 64u], s_y[HBG_SCAN_TB / 64u];
    const uint32_t b = blockIdx.x * HBG_SCAN_TB + threadIdx.x;
    uint32_t x = b < nb ? bcnt[b] : 0u, y = hbg_touched(x), tx, ty;
    tile_scan(&x, &y, &tx, &ty, s_x, s_y);
    if (threadIdx.x == 0) {
        sums[2 * (size_t)blockIdx.x] = tx;
        sums[2 * (size_t)blockIdx.x + 1] = ty;
    }
}

__global__ __launch_bounds__(HBG_SCAN_TB) void k_gather_top(uint32_t *__restrict__ sums, uint32_t ntile,
                                                            uint32_t *__restrict__ ctl) {
    __shared__ uint32_t s_x[HBG_SCAN_TB / 64u], s_y[HBG_SCAN_TB / 64u];
    uint32_t cx = 0, cy = 0;
    for (uint32_t t0 = 0; t0 < ntile; t0 += HBG_SCAN_TB) {
        const uint32_t t = t0 + threadIdx.x;              // (ntile <= 2^22: no overflow)
        const uint32_t vx = t < ntile ? sums[2 * (size_t)t] : 0u, vy = t < ntile ? sums[2 * (size_t)t + 1] : 0u;
        uint32_t x = vx, y = vy, tx, ty;
        tile_scan(&x, &y, &tx, &ty, s_x, s_y);
        if (t < ntile) {
            sums[2 * (size_t)t] = cx + x - vx;
            sums[2 * (size_t)t + 1] = cy + y - vy;
        }
        cx += tx;
        cy += ty;
    }
    if (threadIdx.x == 0) ctl[HB_CTL_WALKS] = cy;
}

__global__ __launch_bounds__(HBG_SCAN_TB) void k_gather_first(const uint32_t *__restrict__ bcnt, uint32_t nb,
                                                              const uint32_t *__restrict__ sums,
                                                              const hh_batch_item *__restrict__ index, uint64_t RB,
                                                              uint32_t *__restrict__ first,
                                                              uint32_t *__restrict__ ctl) {
    __shared__ uint32_t s_x[HBG_SCAN_TB / 64u], s_y[HBG_SCAN_TB / 64u], s_cnt[HBP_BINS];
    const uint32_t tid = threadIdx.x, b = blockIdx.x * HBG_SCAN_TB + tid;
    if (tid < HBP_BINS) s_cnt[tid] = 0;
    const uint32_t c = b < nb ? bcnt[b] : 0u;
    uint32_t x = c, y = hbg_touched(c), tx, ty;
    tile_scan(&x, &y, &tx, &ty, s_x, s_y);               // (its barriers order s_cnt's clearing too)
    if (b < nb) first[b] = sums[2 * (size_t)blockIdx.x] + x - c;
    // (a block with a valid piece has an index entry that keeps the rules)
    if (c) atomicAdd(&s_cnt[hbp_bin(index[b].bits, RB)], 1u);
    __syncthreads();
    if (tid < HBP_BINS && s_cnt[tid]) atomicAdd(&ctl[HB_CTL_CNT + tid], s_cnt[tid]);
}

__global__ __launch_bounds__(HBG_TB) void k_gather_place(uint32_t P, const GatherPiece *__restrict__ pc,
                                                         const uint32_t *__restrict__ ctl,
                                                         const uint32_t *__restrict__ first, uint32_t *cur,
                                                         GatherPiece *__restrict__ list) {
    const uint32_t s = blockIdx.x * HBG_TB + threadIdx.x;
    if (s >= P || s >= ctl[HB_CTL_TOTAL]) return;
    const GatherPiece p = pc[s];
    if (p.blk == HBG_NOBLK) return;
    const uint32_t at = first[p.blk] + atomicAdd(&cur[p.blk], 1u);
    if (at < P) list[at] = p;                             // (always: the counts are of these very pieces)
}

__global__ __launch_bounds__(HBG_TB) void k_gather_walks(uint32_t nb, const uint32_t *__restrict__ bcnt,
                                                         const uint64_t *__restrict__ bend,
                                                         const uint32_t *__restrict__ first,
                                                         const hh_batch_item *__restrict__ index, uint64_t RB,
                                                         uint32_t *__restrict__ ctl, GatherWalk *__restrict__ walks,
                                                         uint32_t nwalk) {
    __shared__ uint32_t s_cnt[HBP_BINS], s_loc[HBP_BINS], s_base[HBP_BINS];
    const uint32_t tid = threadIdx.x, b = blockIdx.x * HBG_TB + tid;
    if (tid < HBP_BINS) {
        s_cnt[tid] = ctl[HB_CTL_CNT + tid];               // (final: k_gather_first is done)
        s_loc[tid] = 0;
    }
    __syncthreads();
    const uint32_t c = b < nb ? bcnt[b] : 0u;
    uint32_t bin = 0, rank = 0;
    uint64_t data_off = 0, bits = 0;
    if (c) {
        data_off = index[b].data_off;
        bits = index[b].bits;
        bin = hbp_bin(bits, RB);
        rank = atomicAdd(&s_loc[bin], 1u);
    }
    __syncthreads();
    if (tid < HBP_BINS)
        s_base[tid] = hbp_start(s_cnt, tid) + (s_loc[tid] ? atomicAdd(&ctl[HB_CTL_CUR + tid], s_loc[tid]) : 0u);
    __syncthreads();
    if (c) {
        const uint32_t at = s_base[bin] + rank;
        if (at < nwalk) walks[at] = GatherWalk{data_off, bits, bend[b], first[b], c};   // (always)
    }
}

__global__ __launch_bounds__(64 * HB_WMAX) void k_gather(const uint8_t *__restrict__ data,
                                                         const GatherWalk *__restrict__ walks,
                                                         const uint32_t *__restrict__ ctl,
                                                         const GatherPiece *__restrict__ list,
                                                         BatchRes *__restrict__ res, uint8_t *__restrict__ out,
                                                         FsmTab tab, BatchGeo geo) {
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
    uint32_t *hitf = chg + 4;                             // a piece has bytes in the round (chg[0..2]: the fix rounds')
    uint8_t *stg = smem + geo.stg_off;
    const bool lds0 = lds_base_is_zero(smem);
    const uint32_t jr = wv * 64u + lane;                  // the lane's region of a round
    const uint64_t RB = (uint64_t)HB_NR * W * S;          // a round's bits
    const uint32_t T = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctl[HB_CTL_WALKS]);

    for (uint32_t it = blockIdx.x; it < T; it += gridDim.x) {
        const uint64_t data_off = uni64(walks[it].data_off), bits = uni64(walks[it].bits);
        const uint64_t end = uni64(walks[it].end);
        const uint32_t lcnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)walks[it].cnt);
        const GatherPiece *pl = list + (uint32_t)__builtin_amdgcn_readfirstlane((int)walks[it].first);
        const uint32_t *g = (const uint32_t *)(data + data_off);
        // (a walk has a piece, and a piece a byte: end > 0)
        const uint64_t nwords = (bits + 31u) / 32u, rounds = end ? (bits + RB - 1u) / RB : 0u;
        uint64_t base = 0;                                // symbols before the round
        uint32_t carry = 0, fail = lds0 ? 0u : 1u;        // the state entering the round
        for (uint64_t rd = 0; rd < rounds; rd++) {
            const uint64_t R0 = rd * RB, R = R0 + (uint64_t)jr * S;
            const __amdgpu_buffer_rsrc_t rs = fs_rsrc(g, R0 / 32u, nwords);
            __syncthreads();                              // the round before has read its rows, its staging and hitf
            uint32_t *row = pay + jr * RW;
#pragma unroll 4
            for (uint32_t k = 0; k < SW; k++) row[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(4u * (jr * SW + k)), 0, 0);
            if (tid == 0) {
                chg[0] = 0;
                *hitf = 0;
            }
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
            if (tot + 8u > geo.stg_bytes) fail = 1u;      // (the host sized it for the most a round holds)
            // does any piece of the block have bytes among the round's [base, base + tot)?
            bool hit = false;
            for (uint32_t j = tid; !fail && j < lcnt; j += blockDim.x) {
                uint32_t from;
                hit |= hb_window(base, tot, pl[j].skip, pl[j].cap, &from) != 0u;
            }
            if (__builtin_amdgcn_ballot_w64(hit) != 0 && lane == 0) *hitf = 1u;
            __syncthreads();
            if (*hitf) {
                // the round once into the staging, its byte t at stg + t
                if (tid == 0) *(uint32_t *)(stg + (tot & ~3u)) = 0u;   // the last, partial dword: ORs only
                BatchSink sink;
                sink.init(smem, geo.stg_off + L);
                hb_bits_init(&b, row, 0);
                uint32_t n2;
                hb_region(&F, &b, nb, whole, at_end, ent, sink, &n2);
                __syncthreads();
                if (sink.sh) atomicOr((uint32_t *)(smem + sink.wd), sink.a);
                __syncthreads();
                // copy-out: 64 pieces at a time, a lane per piece
                for (uint32_t c0 = 0, ch = 0; c0 < lcnt; c0 += 64u, ch++) {
                    const uint32_t j = c0 + lane;
                    const bool mine = ch % W == wv;       // the wave that takes this chunk's short parts and edges
                    uint32_t keep = 0, from = 0;
                    uint64_t dst = 0;
                    if (j < lcnt) {
                        const GatherPiece p = pl[j];
                        keep = hb_window(base, tot, p.skip, p.cap, &from);
                        dst = (uint64_t)(uintptr_t)out + p.out_off + (base + from - p.skip);   // (used when keep != 0 only)
                    }
                    if (mine && keep <= HBG_SMALL) {
                        uint8_t *d = (uint8_t *)(uintptr_t)dst;
                        for (uint32_t p = 0; p < keep; p++) d[p] = stg[from + p];
                    }
                    uint64_t big = __builtin_amdgcn_ballot_w64(keep > HBG_SMALL);
                    while (big) {
                        const int l = __builtin_ctzll(big);
                        big &= big - 1u;
                        const uint32_t kf = (uint32_t)__shfl((int)from, l, 64), kk = (uint32_t)__shfl((int)keep, l, 64);
                        const uint64_t kd = (uint64_t)(uint32_t)__shfl((int)(uint32_t)(dst >> 32), l, 64) << 32 |
                                            (uint32_t)__shfl((int)(uint32_t)dst, l, 64);
                        uint32_t head, body;
                        hbg_copy_split(kd, kk, &head, &body);
                        uint8_t *d = (uint8_t *)(uintptr_t)kd;
                        if (mine) {
                            const uint32_t t0 = head + 16u * body, tail = kk - t0;   // (head, tail < 16)
                            if (lane < head) d[lane] = stg[kf + lane];
                            if (lane < tail) d[t0 + lane] = stg[kf + t0 + lane];
                        }
                        for (uint32_t q = jr; q < body; q += 64u * W) {
                            const uint32_t so = kf + head + 16u * q, sh = (so & 3u) * 8u;
                            const uint32_t *sp = (const uint32_t *)(stg + (so & ~3u));   // (sp[4] ends below tot + 4)
                            const uint32_t w0 = sp[0], w1 = sp[1], w2 = sp[2], w3 = sp[3], w4 = sp[4];
                            u32x4 v;
                            v.x = __builtin_amdgcn_alignbit(w1, w0, sh);
                            v.y = __builtin_amdgcn_alignbit(w2, w1, sh);
                            v.z = __builtin_amdgcn_alignbit(w3, w2, sh);
                            v.w = __builtin_amdgcn_alignbit(w4, w3, sh);
                            *(u32x4 *)(d + head + 16u * q) = v;
                        }
                    }
                }
            }
            base += tot;
            carry = carry_next;
            if (hbg_walk_done(base, end)) break;          // no later round is loaded or walked
        }
        // every piece's result, once, from the symbols seen
        for (uint32_t j = tid; j < lcnt; j += blockDim.x) {
            const uint64_t skip = pl[j].skip, cap = pl[j].cap;
            const uint64_t len = hbg_piece_len(base, skip, cap);
            res[pl[j].slot] = BatchRes{len, hbg_piece_status((int)fail, len, cap)};
        }
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// The resident workgroups of k_gather, asked once per launch shape (device,
// waves, dynamic LDS) and kept here: BatchDev's grid_max is k_batch's.
static std::mutex g_grid_mu;
static struct { int dev; uint32_t W, lds, grid; } g_grid[16];
static uint32_t g_grid_n;

static int gather_grid(const BatchDev *b, uint32_t *grid) {
    int dev = 0;
    FS_OK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_grid_mu);
    for (uint32_t i = 0; i < g_grid_n; i++)
        if (g_grid[i].dev == dev && g_grid[i].W == b->W && g_grid[i].lds == b->lds) {
            *grid = g_grid[i].grid;
            return HH_OK;
        }
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, (const void *)k_gather) != hipSuccess || fa.sharedSizeBytes != 0) return HH_ERR_INTERNAL;
    int per = 0, ncu = 0;
    FS_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_gather, (int)(64 * b->W), b->lds));
    FS_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (per < 1 || ncu < 1) return HH_ERR_UNSUPPORTED;
    *grid = (uint32_t)(per * ncu);
    const uint32_t at = g_grid_n < 16u ? g_grid_n++ : 0u;       // (a full table: the oldest shape is asked again later)
    g_grid[at].dev = dev; g_grid[at].W = b->W; g_grid[at].lds = b->lds; g_grid[at].grid = *grid;
    return HH_OK;
}

// Beside the range read's workspace (whose descriptor arrays hold the piece
// records by slot and by list position): per block its end (8), count, cursor
// and first position (4 each); per 1024 blocks two sums; a walk (32) per block
// that can be touched, min(nb, P).
int batch_decode_gather(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                        const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms,
                        const hh_block_read *d_reads, uint64_t m, uint32_t P, uint32_t nb, void *d_out,
                        uint64_t out_bytes, uint64_t *d_read_len, int32_t *d_status, hh_batch_summary *d_summary,
                        hipStream_t st) {
    if (!b->ok) return HH_ERR_UNSUPPORTED;
    uint32_t grid_max = 0;
    const int grc = gather_grid(b, &grid_max);
    if (grc != HH_OK) return grc;
    if (!b->end) FS_OK(hipEventCreateWithFlags(&b->end, hipEventDisableTiming));
    const uint32_t nwalk = nb < P ? nb : P, ntile = (uint32_t)(((uint64_t)nb + HBG_SCAN_TB - 1u) / HBG_SCAN_TB);
    const size_t rbytes = (read_ws_bytes(m, P) + 15u) & ~(size_t)15u;
    const size_t per_blk = (size_t)nb * 20u, sums = (size_t)ntile * 8u;
    const int wrc = batch_ws(b, rbytes + (size_t)nwalk * sizeof(GatherWalk) + per_blk + sums + 16u, 0);
    if (wrc != HH_OK) return wrc;
    ReadWs w;
    read_ws_carve(&w, b->d_ws, m, P);
    uint8_t *p = (uint8_t *)b->d_ws + rbytes;
    GatherWalk *walks = (GatherWalk *)p;    p += (size_t)nwalk * sizeof(GatherWalk);
    uint64_t *bend = (uint64_t *)p;         p += (size_t)nb * 8u;      // bend, bcnt, cur: cleared together
    uint32_t *bcnt = (uint32_t *)p;         p += (size_t)nb * 4u;
    uint32_t *cur = (uint32_t *)p;          p += (size_t)nb * 4u;
    uint32_t *first = (uint32_t *)p;        p += (size_t)nb * 4u;
    uint32_t *tsum = (uint32_t *)p;
    GatherPiece *pc = (GatherPiece *)w.tmp, *list = (GatherPiece *)w.desc;
    if (b->pend && b->pend_st != st) FS_OK(hipStreamWaitEvent(st, b->end, 0));
    const uint64_t RB = (uint64_t)HB_NR * b->W * fd->S;
    const uint32_t gp = (uint32_t)(((uint64_t)P + HBG_TB - 1u) / HBG_TB);
    int rc = read_count_enqueue(&w, n_syms, block_syms, d_reads, (uint32_t)m, P, out_bytes, d_summary, st);
    // (no blocks: no read has a piece, and ctl's total and walks stay 0)
    if (rc == HH_OK && nb) {
        if (hipMemsetAsync(bend, 0, (size_t)nb * 16u, st) != hipSuccess) rc = HH_ERR_DEVICE;
        if (rc == HH_OK) {
            hipLaunchKernelGGL(k_gather_fill, dim3(gp), dim3(HBG_TB), 0, st, P, (const uint64_t *)w.start, (uint32_t)m,
                               (const hh_block_read *)w.reads, d_index, data_bytes, block_syms, pc, w.key, w.res, w.own,
                               (const uint32_t *)w.ctl, bcnt, bend);
            hipLaunchKernelGGL(k_gather_sums, dim3(ntile), dim3(HBG_SCAN_TB), 0, st, (const uint32_t *)bcnt, nb, tsum);
            hipLaunchKernelGGL(k_gather_top, dim3(1), dim3(HBG_SCAN_TB), 0, st, tsum, ntile, w.ctl);
            hipLaunchKernelGGL(k_gather_first, dim3(ntile), dim3(HBG_SCAN_TB), 0, st, (const uint32_t *)bcnt, nb,
                               (const uint32_t *)tsum, d_index, RB, first, w.ctl);
            hipLaunchKernelGGL(k_gather_place, dim3(gp), dim3(HBG_TB), 0, st, P, (const GatherPiece *)pc,
                               (const uint32_t *)w.ctl, (const uint32_t *)first, cur, list);
            hipLaunchKernelGGL(k_gather_walks, dim3((uint32_t)(((uint64_t)nb + HBG_TB - 1u) / HBG_TB)), dim3(HBG_TB), 0,
                               st, nb, (const uint32_t *)bcnt, (const uint64_t *)bend, (const uint32_t *)first, d_index,
                               RB, w.ctl, walks, nwalk);
            const BatchGeo geo = batch_geo(b, fd, nwalk);
            const FsmTab tab = {fd->ct, fd->b1, fd->tsym, fd->et, fd->er};
            const uint32_t grid = nwalk < grid_max ? nwalk : grid_max;
            hipLaunchKernelGGL(k_gather, dim3(grid), dim3(64 * b->W), b->lds, st, (const uint8_t *)d_data,
                               (const GatherWalk *)walks, (const uint32_t *)w.ctl, (const GatherPiece *)list, w.res,
                               (uint8_t *)d_out, tab, geo);
            if (hipGetLastError() != hipSuccess) rc = HH_ERR_DEVICE;
        }
    }
    if (rc == HH_OK) rc = read_results_enqueue(&w, (uint32_t)m, P, d_read_len, d_status, d_summary, st);
    // (also after a failed launch: what was enqueued before it uses the workspace)
    FS_OK(hipEventRecord(b->end, st));
    b->pend = 1;
    b->pend_st = st;
    return rc;
}
