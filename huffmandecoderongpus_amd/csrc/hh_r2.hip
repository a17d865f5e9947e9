// hh_r2.hip -- the legacy two-pass decode (HH_FLAG_LEGACY, and trees the state
// machine does not take): its kernels, their launch sizing and decode_fast.
//
// The decode is four launches on one stream, no in-kernel waits between
// workgroups (O(N) memory, 64-bit offsets):
//
//   k_front   one tile (HH_NR = 64 regions x S bits) per WAVE at a time,
//             persistent grid, independent of every other tile and wave:
//               stage     the tile's words (+ the next tile's first HH_KM
//                         regions and a halo), prefetched one tile ahead into
//                         registers, stored to the wave's LDS slice transposed
//               pass 1    every lane decodes its region from a G-bit overlap
//                         head: count, exit and boundary mask (decodeallbits)
//               walks     each exit that did not merge in the overlap window
//                         is walked against the next regions' chains until
//                         they share a boundary (makebigtable)
//               table     charged count and leaving state for every entering
//                         state d < HH_KM -> workspace; one 32-bit record per
//                         lane (regions crossed, entry offset, correction,
//                         count) -> workspace
//   k_scan1/2 the state entering every tile (the predecessor's leaving state,
//             composed through the tables back to the nearest CONST tile) and
//             the exclusive prefix of the tiles' charged counts
//             (calcbitsindex / findmax)
//   k_emit    one tile per WAVE at a time again: live lanes from the tile's
//             entering state, run offsets by a wave scan, each lane
//             re-decodes its exact run into the wave's LDS staging buffer,
//             copied out with 16-B stores (calcresult)
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hh_algo.h"
#include "hh_dec.h"
#include "hh_internal.h"
#include "hiphuff.h"

#ifndef HH_FW
#define HH_FW 8                     // waves per workgroup (k_front), sharing the 16 KiB F: 3
                                    // workgroups per CU (with the 13-bit F, 4 / 7 / 8 / 14 waves:
                                    // front + walks 1.29 / 1.21 / 1.13 / 1.26 ms)
#endif
#define HH_SCAN_TB 1024             // tiles per k_scan1 block
#define HH_SCAN_BACK 4096           // longest non-CONST chain k_scan1 composes (else host scan)

// flags[0]: status bits; [2..3] total symbols (u64); [4..9] first failed walk;
// [12] a prologue tile is CONST; [13] an emitted tile is CONST; [14] state
// leaving the last tile; [15] state entering the first emitted tile
enum { F_FAIL = 1, F_OVER = 2, F_SCAN = 4 };

// Per-lane record of the front pass (k_front -> k_emit), 32 bits:
//   bits 0..2 k-1 (regions the lane's walk crossed), 3..7 e (the walk's first
//   boundary in the merge region, < 32), 8..17 delta (signed), 18..29 n + cov
//   (own symbols + symbols of covered regions)
__device__ __forceinline__ uint32_t rec_pack(uint32_t k, uint32_t e, int32_t delta, uint32_t nc) {
    return (k - 1u) | (e << 3) | (((uint32_t)delta & 0x3ffu) << 8) | (nc << 18);
}
__device__ __forceinline__ uint32_t rec_k(uint32_t r) { return (r & 7u) + 1u; }
__device__ __forceinline__ uint32_t rec_e(uint32_t r) { return (r >> 3) & 31u; }
__device__ __forceinline__ int32_t rec_delta(uint32_t r) { return (int32_t)(r << 14) >> 22; }
__device__ __forceinline__ uint32_t rec_nc(uint32_t r) { return r >> 18; }

struct Geometry {
    uint64_t bits;       // stream length
    uint64_t nwords;     // readable payload words
    uint64_t ntiles;
    uint32_t S, sw;
    uint32_t maxadv;     // max(HH_P, longest code)
    uint32_t G;          // overlap bits (hh_region_head)
    uint32_t in_state;   // state entering tile 0 (a shard's entry; 0 at the stream start)
    uint64_t emit_from;  // tiles before this one are a prologue: decoded for their
                         // leaving state only (a shard's probe of its predecessor)
    uint32_t fwalk;      // lookups of a walk in k_front (longer: deferred to k_walk)
    uint32_t nfw;        // k_front's waves (each with its list of deferred walks)
    uint64_t qcap;       // entries per list (the wave's tiles x HH_NR)
    uint32_t xcap;       // k_emit: deferred runs per wave's list (HH_XPT per tile)
};

// Workspace carve (decode_fast).  Nothing but `flags` needs zeroing: every
// other word is written before it is read.
struct Work {
    uint32_t *flags;     // 64 B
    uint64_t *tabs;      // [ntiles][HH_KM] rows: count | state << 20; row 0 bit 61 = CONST
    uint32_t *recs;      // [ntiles][HH_NR] lane records (a group's are contiguous)
    uint32_t *st;        // [ntiles + 1] state entering each tile (st[ntiles]: leaving the last)
    int32_t *lex;        // [ntiles + 1] exclusive prefix of charged counts within its scan block
    int64_t *blk;        // [nblk] scan block totals, then exclusive block bases
    uint64_t *q;         // [nfw][qcap] deferred walks of each k_front wave: tile * HH_NR + lane |
                         // (exit | count << 16) << 32
    uint32_t *qn;        // [nfw] their counts
    uint32_t *xn;        // [ntiles * HH_NR] pass-1 exit | count << 16 of every region
    uint64_t *xq;        // [k_emit waves][xcap] deferred runs: output offset, tile << 32 | entry | end << 16
    uint32_t *xqn;       // [k_emit waves] their counts
};

// ---------------------------------------------------------------------------
// wave / block helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t wave_incl_scan(int32_t x) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    return x;
}

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Exclusive block scan of int32 over NT threads; *total = block sum.
template <uint32_t NT>
__device__ __forceinline__ int32_t block_excl_scan(int32_t v, int32_t *s_tmp, int32_t *total) {
    constexpr uint32_t NW = NT / 64;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const int32_t x = wave_incl_scan(v);
    if (lane == 63) s_tmp[wv] = x;
    __syncthreads();
    int32_t base = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < NW; i++) {
        const int32_t t = s_tmp[i];
        base += i < wv ? t : 0;
        tot += t;
    }
    *total = tot;
    __syncthreads();
    return base + x - v;
}

// Words of a staged span through a buffer resource over its readable words:
// the range check returns 0 past the payload, so no lane branches between
// load paths (with a per-lane branch the compiler waits for every load in
// flight before the second path's loads).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t words_rsrc(const uint32_t *g, uint64_t tw0, uint64_t nok) {
    const uint64_t left = nok > tw0 ? nok - tw0 : 0u;
    const uint32_t nbytes = left > 0x3fffffffull ? 0xfffffffcu : (uint32_t)left * 4u;
    return __builtin_amdgcn_make_buffer_rsrc((void *)(g + tw0), 0, (int)nbytes, 0x00020000);
}

template <uint32_t sw>
__device__ __forceinline__ void load_region(uint32_t *v, __amdgpu_buffer_rsrc_t r, uint32_t col) {
    const uint32_t v0 = 4u * col * sw;
    if (sw % 4 == 0) {
#pragma unroll
        for (uint32_t k = 0; k < HH_SW_MAX; k += 4) {
            if (k < sw) {
                const u32x4 q = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(v0 + 4u * k), 0, 0));
                v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < HH_SW_MAX; k++)
            if (k < sw) v[k] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)(v0 + 4u * k), 0, 0);
    }
}

// Registers holding one tile's words for this lane: its region column and up
// to two words of the columns past the tile (the next tile's first HH_KM
// regions and the halo).
static_assert((HH_NCOL - HH_NR) * HH_SW_MAX <= 2 * 64, "a tile's extra columns: two words per lane");
static_assert(HH_NLS >= HH_NCOL && HH_NLS % 16 == 0, "LDS column stride");
struct Prefetch {
    uint32_t v[HH_SW_MAX];
    uint32_t halo, halo2;
};

// a wave's tile (lane = its region)
template <uint32_t sw>
__device__ __forceinline__ void prefetch_wtile(Prefetch &pf, const uint32_t *g, uint64_t tw0, uint64_t nok) {
    const uint32_t j = threadIdx.x & 63u;
    const __amdgpu_buffer_rsrc_t r = words_rsrc(g, tw0, nok);
    load_region<sw>(pf.v, r, j);
    constexpr uint32_t nx = (HH_NCOL - HH_NR) * sw;
    pf.halo = j < nx ? __builtin_amdgcn_raw_buffer_load_b32(r, (int)(4u * (HH_NR * sw + j)), 0, 0) : 0u;
    pf.halo2 = j + 64 < nx ? __builtin_amdgcn_raw_buffer_load_b32(r, (int)(4u * (HH_NR * sw + j + 64)), 0, 0) : 0u;
}
template <uint32_t sw>
__device__ __forceinline__ void store_wtile(const Prefetch &pf, uint32_t *s_w) {
    const uint32_t j = threadIdx.x & 63u;
    constexpr uint32_t nx = (HH_NCOL - HH_NR) * sw;
#pragma unroll
    for (uint32_t k = 0; k < HH_SW_MAX; k++)
        if (k < sw) s_w[k * HH_NLS + j] = pf.v[k];
    if (j < nx) s_w[(j % sw) * HH_NLS + HH_NR + j / sw] = pf.halo;
    if (j + 64 < nx) s_w[((j + 64) % sw) * HH_NLS + HH_NR + (j + 64) / sw] = pf.halo2;
}

// Lanes of one wave exchanging values through LDS: a wave's LDS operations
// execute in order, so a compiler fence is all the ordering needed.
#define WAVE_SYNC()                                                    \
    do {                                                               \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         \
        __builtin_amdgcn_wave_barrier();                               \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");         \
    } while (0)

// Live masks over the entering state d of a wave's tile (bit d of mem: the
// lane is live when the tile is entered in region d): hh_mem_init, then the
// walks with k > 1 (exceptions), in ascending lane order, clear the lanes
// they cover (within the tile).  s_k, s_mem: the wave's 64 entries.  One
// lane; a tile rarely has more than one exception.
__device__ __forceinline__ uint32_t resolve_live_wave(uint32_t kk, uint8_t *s_k, uint8_t *s_mem) {
    const uint32_t j = threadIdx.x & 63u;
    const uint64_t ex = __ballot(kk > 1);
    if (ex == 0) return hh_mem_init(j);
    s_k[j] = (uint8_t)kk;
    s_mem[j] = (uint8_t)hh_mem_init(j);
    WAVE_SYNC();
    if (j == 0) {
        uint64_t m = ex;
        while (m) {
            const uint32_t e = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t ke = s_k[e];
            const uint8_t me = s_mem[e];
            for (uint32_t q = e + 1; q < e + ke && q < HH_NR; q++) s_mem[q] &= (uint8_t)~me;
        }
    }
    WAVE_SYNC();
    return s_mem[j];
}

// The front's tables into LDS: F, its escape directory, L2.
__device__ __forceinline__ void load_ftables(const DevTab &tab, uint16_t *s_f, uint32_t *s_fdir, uint32_t *s_l2) {
    const uint32_t *f32 = (const uint32_t *)tab.f;
    for (uint32_t i = threadIdx.x; i < HH_F_SIZE / 2; i += blockDim.x) ((uint32_t *)s_f)[i] = f32[i];
    for (uint32_t i = threadIdx.x; i < tab.fdir_used; i += blockDim.x) s_fdir[i] = tab.fdir[i];
    for (uint32_t i = threadIdx.x; i < tab.l2_used; i += blockDim.x) s_l2[i] = tab.l2[i];
}
__host__ __device__ constexpr uint32_t ftab_words(uint32_t fdir, uint32_t l2) {
    return HH_F_SIZE / 2 + ((fdir + 3u) & ~3u) + ((l2 + 3u) & ~3u);
}

#ifndef HH_FRONT_MINB
#define HH_FRONT_MINB 2   // workgroups per CU the front kernel's registers are sized for (it
                          // compiles to ~70 VGPRs: up to 7 waves per SIMD; its LDS allows 6)
#endif

// Diagnostic build only (-DHH_DIAG): every wave stamps the shader clock
// between the front kernel's phases and adds the cycles into dbg[phase]
// (0 staging, 4 own pass 1, 1 its barrier wait, 5 own walks, 2 their barrier
// wait, 3 table); walk statistics go to dbg[8..]: lanes, lookups, the sum over
// tiles of the longest walk, the longest walk.  hh_debug_counters reads them.
#ifdef HH_DIAG
#define DIAG_DECL uint64_t dg_acc[6] = {0, 0, 0, 0, 0, 0}, dg_w[4] = {0, 0, 0, 0}; uint64_t dg_t = __builtin_amdgcn_s_memtime();
#define DIAG_STAMP(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); dg_acc[i] += t_ - dg_t; dg_t = t_; } while (0)
#define DIAG_FLUSH(dbg) do { if ((threadIdx.x & 63u) == 0) for (int i_ = 0; i_ < 6; i_++) atomicAdd((unsigned long long *)&(dbg)[i_], (unsigned long long)dg_acc[i_]); \
    if ((threadIdx.x & 63u) == 0) { for (int i_ = 0; i_ < 3; i_++) atomicAdd((unsigned long long *)&(dbg)[8 + i_], (unsigned long long)dg_w[i_]); \
        atomicMax((unsigned long long *)&(dbg)[11], (unsigned long long)dg_w[3]); } } while (0)
#define EDIAG_DECL uint64_t eg_acc[5] = {0, 0, 0, 0, 0}; uint64_t eg_t = __builtin_amdgcn_s_memtime();
#define EDIAG_STAMP(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); eg_acc[i] += t_ - eg_t; eg_t = t_; } while (0)
#define EDIAG_FLUSH(dbg) do { if ((threadIdx.x & 63u) == 0) { const int ix_[5] = {6, 7, 12, 13, 14}; \
    for (int i_ = 0; i_ < 5; i_++) atomicAdd((unsigned long long *)&(dbg)[ix_[i_]], (unsigned long long)eg_acc[i_]); } } while (0)
#else
#define DIAG_DECL
#define DIAG_STAMP(i) do {} while (0)
#define DIAG_FLUSH(dbg) do {} while (0)
#define EDIAG_DECL
#define EDIAG_STAMP(i) do {} while (0)
#define EDIAG_FLUSH(dbg) do {} while (0)
#endif

// ---------------------------------------------------------------------------
// k_front: pass 1 and the short walks of every tile, one tile per wave at a
// time (a persistent grid; wave gw takes tiles gw, gw + #waves, ...).  Within
// a tile the lanes exchange values through the wave's own LDS slice, never
// with other waves: no workgroup barrier after the tables.  A walk longer
// than geo.fwalk lookups is deferred to k_walk (a wave would otherwise wait
// for its longest walk: kjv's average walk is 0.5 lookups, a wave's longest
// 16); the tables follow from the records in k_table.
// ---------------------------------------------------------------------------
template <uint32_t SW>
__global__ __launch_bounds__(64 * HH_FW, HH_FRONT_MINB) void k_front(const uint32_t *__restrict__ gdata, Geometry geo,
                                                                 DevTab tab, Work wk, uint64_t *dbg) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ uint32_t s_ya[HH_FW][HH_NR];    // entry points of the regions' own chains

    constexpr uint32_t S = 32 * SW;
    const uint32_t j = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint16_t *s_f = (uint16_t *)smem;                   // F, its escape directory, L2 (shared),
    uint32_t *s_fdir = (uint32_t *)smem + HH_F_SIZE / 2;
    uint32_t *s_l2 = s_fdir + ((tab.fdir_used + 3u) & ~3u);
    uint32_t *s_w = (uint32_t *)smem + ftab_words(tab.fdir_used, tab.l2_used) + wv * (SW * HH_NLS);
    uint32_t *s_y = s_ya[wv];                           // then the waves' slices (SW * HH_NLS words)

    const uint64_t tile_bits = (uint64_t)HH_NR * S;
    const uint32_t span = HH_NCOL * S;                  // bits staged per tile
    load_ftables(tab, s_f, s_fdir, s_l2);
    __syncthreads();                                    // (the only workgroup barrier)

    hh_ctx c;
    c.w = s_w;
    c.sw = SW;
    c.nls = HH_NLS;
    c.magic = 0;
    c.l1m = nullptr;
    c.l1s = nullptr;
    c.l1 = nullptr;
    c.f = s_f;
    c.fdir = s_fdir;
    c.pf = HH_PF;
    c.l2 = s_l2;
    c.tree = tab.tree;
    c.tsym = tab.tsym;
    c.maxadv = geo.maxadv > HH_PF ? geo.maxadv : HH_PF;
    c.G = geo.G;

    // The next tile's words are loaded one tile ahead into registers and
    // stored to LDS once the walks are done (before the tile's record
    // stores: vmcnt retires in order and counts stores too).  The loads run
    // unconditionally (the last tile again past the end): a conditional load
    // merges two values, which the compiler waits for.
    const uint64_t nwv = (uint64_t)gridDim.x * HH_FW;
    const uint64_t tlast = geo.ntiles ? geo.ntiles - 1 : 0;
    auto clampt = [&](uint64_t tt) { return tt < tlast ? tt : tlast; };
    Prefetch pf;
    uint64_t t = (uint64_t)blockIdx.x * HH_FW + wv;
    // deferred walks: this wave's list q[qbase, qbase + qn), its length -> qn[gw]
    const uint32_t gw = (uint32_t)t;
    const uint64_t qbase = (uint64_t)gw * geo.qcap;
    uint32_t qn = 0;
    if (t < geo.ntiles) {
        prefetch_wtile<SW>(pf, gdata, t * tile_bits / 32, geo.nwords);
        store_wtile<SW>(pf, s_w);
        prefetch_wtile<SW>(pf, gdata, clampt(t + nwv) * tile_bits / 32, geo.nwords);
    }
    DIAG_DECL
    for (; t < geo.ntiles; t += nwv) {
        WAVE_SYNC();                                    // this tile's words stored
        const uint64_t rem = geo.bits - t * tile_bits;
        c.bt = rem < span ? (uint32_t)rem : span;
        const uint32_t bt = c.bt;
        DIAG_STAMP(0);

        // pass 1: the head (from G bits before the region, lanes > 0), then
        // the own chain from its entry point y, counted
        const uint32_t p0 = j * S;
        uint32_t n = 0, x = bt, y = bt;
        if (p0 < bt) {
            y = j > 0 && c.G ? hh_region_head(&c, p0 - c.G, p0, nullptr) : p0;
            const uint32_t lim = p0 + S < bt ? p0 + S : bt;
            x = y < lim ? hh_region_count(&c, y, lim, &n) : y;
        }
        s_y[j] = y;
        DIAG_STAMP(1);
        // chain j's exit is chain j+1's entry point: merged there, no walk
        // (the next tile's region 0 is entered at its start)
        const uint32_t R1 = (j + 1) * S;
        const uint32_t yn = (uint32_t)__shfl_down((int)y, 1, 64);
        const bool merged = R1 < bt && x == (j == 63u ? R1 : yn);
        WAVE_SYNC();                                    // s_y complete

        // walks: region j's exit against the next regions' own chains, two
        // pointers, at most geo.fwalk lookups here
        hh_wk w = {1u, x - R1, 0u, 0, 0u, 0u};
        if (!merged) {
            if (geo.fwalk) w = hh_walk(&c, j, S, x, nullptr, nullptr, nullptr, 0, geo.fwalk, s_y, HH_NR);
            else w.more = 1u;                           // (every walk to k_walk)
        }
        const uint32_t rec = rec_pack(w.k ? w.k : 1u, w.e, w.delta, n + w.cov);
        if (w.more) {
            const uint64_t dm = __ballot(1);            // (the deferring lanes)
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
            wk.q[qbase + qn + rank] = (uint64_t)(t * HH_NR + j) | ((uint64_t)(x | (n << 16)) << 32);
        }
        {
            // the wave's own list (an atomic on one counter per deferring
            // wave serialises: 4 ms per decode)
            const uint64_t dm = __ballot(w.more);
            qn += (uint32_t)__builtin_popcountll(dm);
        }
        if (!w.more && w.k == 0) {
            atomicOr(wk.flags, (uint32_t)F_FAIL);
            if (atomicCAS(&wk.flags[4], 0u, 1u) == 0u) {
                wk.flags[5] = (uint32_t)t; wk.flags[6] = j; wk.flags[7] = x; wk.flags[8] = n; wk.flags[9] = bt;
            }
        }
#ifdef HH_DIAG
        {
            const uint32_t st = w.steps;
            uint32_t mx = st;
            uint64_t sm = st;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
                sm += (uint32_t)__shfl_xor((int)(uint32_t)sm, o, 64);
            }
            dg_w[0] += 64;
            dg_w[1] += sm;
            dg_w[2] += mx;
            dg_w[3] = dg_w[3] > mx ? dg_w[3] : mx;
        }
#endif
        DIAG_STAMP(2);
        // the walks are done: the next tile's words go to LDS now, and the
        // tile after it is loaded
        WAVE_SYNC();
        store_wtile<SW>(pf, s_w);
        prefetch_wtile<SW>(pf, gdata, clampt(t + 2 * nwv) * tile_bits / 32, geo.nwords);
        wk.recs[t * HH_NR + j] = rec;                 // (a deferred lane's: k_walk's)
        wk.xn[t * HH_NR + j] = x | (n << 16);         // the region's exit and count, for k_walk
        DIAG_STAMP(3);
    }
    if (j == 0) wk.qn[gw] = qn;
    DIAG_FLUSH(dbg);
}

// ---------------------------------------------------------------------------
// k_walk: the deferred walks (k_front's lists), one lane each: exit
// comparisons (hh_walk_exits, restated here region by region) against the
// regions' pass-1 exits and counts (xn).  A lane stages only the words of
// the region it walks (from G bits before it, for the heads of regions that
// were not decoded, to a halo past it) at LDS index (q * HH_WALK_T + lane).
// The lane's record replaces k_front's placeholder.
// The merge/delta rule here must stay the one of hh_walk_exits (hh_algo.h),
// which the emulator checks against the mask walk: a change to either is a
// change to both (the GPU parity tests with HH_FLAG_LEGACY cover this copy:
// test_walk_bound_and_deferral_lists, test_fixture_legacy_pipeline).
// ---------------------------------------------------------------------------
#ifndef HH_WALK_T
#define HH_WALK_T 256   // lanes per k_walk workgroup (64: +0.05 ms; 512: same)
#endif
template <uint32_t SW>
struct WalkWin {
    static constexpr uint32_t n = SW + 6;   // words of one region's window
};

template <uint32_t SW>
__device__ __forceinline__ void walk_win_load(uint32_t (&v)[WalkWin<SW>::n], const uint32_t *gdata, uint64_t gw0,
                                              uint64_t glim) {
#pragma unroll
    for (uint32_t q = 0; q < WalkWin<SW>::n; q++) {
        const uint64_t gi = gw0 + q;
        v[q] = gdata[gi < glim ? gi : glim - 1];   // (past the payload: past the stream end, unused)
    }
}

template <uint32_t SW>
__global__ __launch_bounds__(HH_WALK_T) void k_walk(const uint32_t *__restrict__ gdata, Geometry geo, DevTab tab, Work wk) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr uint32_t S = 32 * SW, NW = WalkWin<SW>::n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint16_t *s_f = (uint16_t *)smem;                   // F, its escape directory, L2
    uint32_t *s_fdir = (uint32_t *)smem + HH_F_SIZE / 2;
    uint32_t *s_l2 = s_fdir + ((tab.fdir_used + 3u) & ~3u);
    uint32_t *s_win = (uint32_t *)smem + ftab_words(tab.fdir_used, tab.l2_used) + tid;   // NW words
    load_ftables(tab, s_f, s_fdir, s_l2);
    __syncthreads();
    const uint64_t tile_bits = (uint64_t)HH_NR * S;
    const uint32_t span = HH_NCOL * S;
    hh_ctx c;
    c.sw = 1024;                                        // hh_idx(g) = g * HH_WALK_T (below)
    c.nls = HH_WALK_T;
    c.magic = 0;
    c.l1m = nullptr;
    c.l1s = nullptr;
    c.l1 = nullptr;
    c.f = s_f;
    c.fdir = s_fdir;
    c.pf = HH_PF;
    c.l2 = s_l2;
    c.tree = tab.tree;
    c.tsym = tab.tsym;
    c.maxadv = geo.maxadv > HH_PF ? geo.maxadv : HH_PF;
    c.G = geo.G;
    // one k_front wave's list at a time, its entries over the wave's lanes;
    // the next entry is loaded one walk ahead
    const uint32_t nwv = gridDim.x * (HH_WALK_T / 64);
    uint32_t fw = blockIdx.x * (HH_WALK_T / 64) + (tid >> 6), i = lane, cnt = fw < geo.nfw ? wk.qn[fw] : 0u;
    auto next_entry = [&](uint64_t &e) -> bool {
        while (i >= cnt && fw < geo.nfw) {
            i -= cnt;
            fw += nwv;
            cnt = fw < geo.nfw ? wk.qn[fw] : 0u;
        }
        if (fw >= geo.nfw) return false;
        e = wk.q[(uint64_t)fw * geo.qcap + i];
        i += 64;
        return true;
    };
    uint32_t pre[NW];
    uint64_t en = 0;
    bool have_n = next_entry(en);
    while (have_n) {
        const uint64_t ent = en;
        have_n = next_entry(en);
        const uint32_t gl = (uint32_t)ent;
        const uint64_t t = gl / HH_NR;
        const uint32_t j = gl % HH_NR;
        const uint32_t r0 = (uint32_t)(ent >> 32);
        const uint64_t rem = geo.bits - t * tile_bits;
        c.bt = rem < span ? (uint32_t)rem : span;
        const uint32_t bt = c.bt;
        const uint64_t tw0 = t * tile_bits / 32;
        auto win0 = [&](uint32_t k) { const uint32_t g = (j + k) * SW; return g >= 2 ? g - 2 : 0u; };
        walk_win_load<SW>(pre, gdata, tw0 + win0(1), geo.nwords);
        // the regions' pass-1 exits and counts, all loaded at once (a tile
        // past the decoded ones, at a range's end: decoded below)
        const bool nxt_ok = t + 1 < geo.ntiles;
        uint32_t xv[HH_KM + 1];
#pragma unroll
        for (uint32_t k = 1; k <= HH_KM; k++) xv[k] = wk.xn[gl + k];   // (xn has a tile of slack)
        uint32_t A = r0 & 0xffffu, ca = 0;
        A = A < bt ? A : bt;
        hh_wk w = {0u, 0u, 0u, 0, 0u, 0u};
        for (uint32_t k = 1; k <= HH_KM; k++) {
            const uint32_t g0 = win0(k);
            // (most walks end in their first region: the next region's words
            // are loaded only when the walk goes on -- loading them ahead
            // doubled k_walk's HBM reads)
            if (k > 1) walk_win_load<SW>(pre, gdata, tw0 + g0, geo.nwords);
#pragma unroll
            for (uint32_t q = 0; q < NW; q++) s_win[q * HH_WALK_T] = pre[q];
            c.w = s_win - (int32_t)g0 * (int32_t)HH_WALK_T;                  // tile word g at (g - g0)
            const uint32_t rg = j + k, R = rg * S;
            const uint32_t Ec = R + S < bt ? R + S : bt;
            // the region's own chain: its pass-1 exit and count (a tile past
            // the decoded ones, at a range's end: decoded here)
            uint32_t xk, nk;
            if (rg < HH_NR || nxt_ok) {
                const uint32_t v = xv[k];
                xk = (v & 0xffffu) + (rg >= HH_NR ? HH_NR * S : 0u);
                nk = v >> 16;
            } else {
                uint32_t yy = R < bt ? R : bt;
                nk = 0;
                if (R < bt && c.G && rg % HH_NR) yy = hh_region_head(&c, R - c.G, R, nullptr);
                xk = yy < Ec ? hh_region_count(&c, yy, Ec, &nk) : yy;
            }
            const uint32_t e = A > R ? A - R : 0u;
            uint32_t n = 0;
            if (A < Ec) A = hh_region_count(&c, A, Ec, &n);
            if (A == (xk < bt ? xk : bt)) {
                w.k = k;
                w.e = e;
                w.cov = ca;
                w.delta = (int32_t)n - (int32_t)nk;
                break;
            }
            ca += n;
        }
        if (w.k == 0) {
            atomicOr(wk.flags, (uint32_t)F_FAIL);
            if (atomicCAS(&wk.flags[4], 0u, 1u) == 0u) {
                wk.flags[5] = (uint32_t)t; wk.flags[6] = j; wk.flags[7] = r0 & 0xffffu; wk.flags[8] = r0 >> 16; wk.flags[9] = bt;
            }
        } else {
            wk.recs[gl] = rec_pack(w.k, w.e, w.delta, (r0 >> 16) + w.cov);
        }
    }
}

// ---------------------------------------------------------------------------
// k_table: the transfer table of every tile from its lane records, one tile
// per wave: live masks over the entering state d < HH_KM, the charged count
// of the live lanes and the state leaving the tile (from the last live lane,
// the one whose walk crosses the tile end); CONST when the leaving state
// does not depend on d.
// ---------------------------------------------------------------------------
#define HH_TABLE_W 4
__global__ __launch_bounds__(64 * HH_TABLE_W) void k_table(Geometry geo, Work wk) {
    __shared__ uint8_t s_ka[HH_TABLE_W][HH_NR];
    __shared__ uint8_t s_mema[HH_TABLE_W][HH_NR];
    __shared__ int32_t s_cda[HH_TABLE_W][HH_KM];
    __shared__ uint32_t s_osta[HH_TABLE_W][HH_KM];
    const uint32_t j = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    int32_t *s_cd = s_cda[wv];
    uint32_t *s_ost = s_osta[wv];
    const uint64_t step = (uint64_t)gridDim.x * HH_TABLE_W;
    uint64_t t = (uint64_t)blockIdx.x * HH_TABLE_W + wv;
    const uint64_t tlast = geo.ntiles - 1;
    // records loaded two tiles ahead
    auto clampt = [&](uint64_t tt) { return tt < tlast ? tt : tlast; };
    uint32_t rec_n = t < geo.ntiles ? wk.recs[t * HH_NR + j] : 0u;
    uint32_t rec_n2 = t < geo.ntiles ? wk.recs[clampt(t + step) * HH_NR + j] : 0u;
    for (; t < geo.ntiles; t += step) {
        const uint32_t rec = rec_n;
        rec_n = rec_n2;
        rec_n2 = wk.recs[clampt(t + 2 * step) * HH_NR + j];
        const uint32_t kk = rec_k(rec), e = rec_e(rec);
        const int32_t delta = rec_delta(rec);
        const int32_t charged = (int32_t)rec_nc(rec) + delta;
        if (__ballot(kk > 1) == 0) {
            // no exceptions: lane j is live for entering d <= j (all d from
            // lane HH_KM - 1 on), so row d counts the lanes >= d; the last
            // lane leaves the tile for every d (CONST)
            const int32_t incl = wave_incl_scan(charged);
            const int32_t tot = __builtin_amdgcn_readlane(incl, 63);
            const uint32_t os = hh_state_pack(kk - 1u, e, delta);          // (lane 63: j + kk - HH_NR)
            const uint32_t os63 = (uint32_t)__builtin_amdgcn_readlane((int)os, 63);
            if (j < HH_KM)
                wk.tabs[t * HH_KM + j] = hh_tab_pack(tot - (incl - charged), os63) | (j == 0 ? HH_CST : 0ull);
            continue;
        }
        const uint32_t mem = resolve_live_wave(kk, s_ka[wv], s_mema[wv]);
        if (j < HH_KM) s_cd[j] = 0;
        WAVE_SYNC();
        if (j + kk >= HH_NR) {
            const uint32_t os = hh_state_pack(j + kk - HH_NR, e, delta);
#pragma unroll
            for (uint32_t d = 0; d < HH_KM; d++)
                if ((mem >> d) & 1u) s_ost[d] = os;
        }
        // lanes live for every entering d: one wave sum; the few others
        // (lanes < HH_KM, covered lanes): per-d LDS atomics
        const uint32_t full = (1u << HH_KM) - 1u;
        const int32_t v = wave_sum(mem == full ? charged : 0);
        if (mem != full) {
#pragma unroll
            for (uint32_t d = 0; d < HH_KM; d++)
                if ((mem >> d) & 1u) atomicAdd(&s_cd[d], charged);
        }
        WAVE_SYNC();
        const uint32_t dd = j < HH_KM ? j : 0u;
        const int32_t cnt = s_cd[dd] + v;
        const uint32_t os = s_ost[dd];
        // CONST: the leaving state is the same for every entering d
        const bool cst = __ballot(j < HH_KM && os != s_ost[0]) == 0;
        if (j < HH_KM) wk.tabs[t * HH_KM + j] = hh_tab_pack(cnt, os) | (j == 0 && cst ? HH_CST : 0ull);
        WAVE_SYNC();                                    // s_cd / s_ost read before the next tile
    }
}

// ---------------------------------------------------------------------------
// k_scan1 / k_scan2: entering states and output bases of every tile
// ---------------------------------------------------------------------------
// One thread per tile t in [0, ntiles] (t == ntiles: the state leaving the
// last tile).  The state entering t is the leaving state of the nearest
// CONST tile v < t, carried through the tables of v+1 .. t-1 (every tile of a
// natural code is CONST: v = t - 1).  Block-local exclusive prefix of the
// tiles' charged counts -> lex, block total -> blk.
__global__ __launch_bounds__(HH_SCAN_TB) void k_scan1(Geometry geo, Work wk) {
    __shared__ int32_t s_tmp[HH_SCAN_TB / 64];
    __shared__ uint32_t s_cf;
    const uint64_t t = (uint64_t)blockIdx.x * HH_SCAN_TB + threadIdx.x;
    const bool valid = t <= geo.ntiles;
    uint32_t s = geo.in_state;
    int32_t cnt = 0;
    bool cst = false;
    if (valid) {
        if (t > 0) {
            int64_t v = (int64_t)t - 1;
            uint32_t back = 0;
            while (v >= 0 && !(wk.tabs[(uint64_t)v * HH_KM] & HH_CST) && back < HH_SCAN_BACK) {
                v--;
                back++;
            }
            if (back >= HH_SCAN_BACK) {
                atomicOr(wk.flags, (uint32_t)F_SCAN);   // the host composes the chain instead
            } else {
                s = v >= 0 ? hh_tab_state(wk.tabs[(uint64_t)v * HH_KM]) : geo.in_state;
                for (uint64_t u = (uint64_t)(v + 1); u < t; u++)
                    s = hh_tab_state(wk.tabs[u * HH_KM + (hh_state_d(s) & (HH_KM - 1u))]);
            }
        }
        wk.st[t] = s;
        if (t < geo.ntiles) {
            const uint64_t row = wk.tabs[t * HH_KM + (hh_state_d(s) & (HH_KM - 1u))];
            cst = (wk.tabs[t * HH_KM] & HH_CST) != 0;
            cnt = hh_tab_count(row);
            // a prologue tile emits nothing; the last one carries the entry
            // correction of the first emitted tile, so that its base is 0
            if (t < geo.emit_from) cnt = t + 1 == geo.emit_from ? hh_state_delta(hh_tab_state(row)) : 0;
        }
    }
    // CONST seen in the prologue / in the emitted tiles: one atomic per
    // block (one per wave on a single address serialises at the L2)
    const uint64_t mp = __ballot(cst && t < geo.emit_from), me = __ballot(cst && t >= geo.emit_from);
    if (threadIdx.x == 0) s_cf = 0u;
    __syncthreads();
    if ((threadIdx.x & 63u) == 0 && (mp | me)) atomicOr(&s_cf, (mp ? 1u : 0u) | (me ? 2u : 0u));
    int32_t tot;
    const int32_t ex = block_excl_scan<HH_SCAN_TB>(cnt, s_tmp, &tot);   // (barriers inside)
    if (threadIdx.x == 0) {
        if (s_cf & 1u) atomicOr(&wk.flags[12], 1u);
        if (s_cf & 2u) atomicOr(&wk.flags[13], 1u);
    }
    if (valid) wk.lex[t] = ex;
    if (threadIdx.x == 0) wk.blk[blockIdx.x] = tot;
}

// One block: exclusive scan of the block totals (int64) into block bases,
// starting from the stream-entry correction; the decode's totals.
__global__ __launch_bounds__(1024) void k_scan2(Geometry geo, Work wk, uint32_t nblk) {
    __shared__ int64_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    int64_t carry = geo.emit_from ? 0 : (int64_t)hh_state_delta(geo.in_state);
    for (uint32_t b0 = 0; b0 < nblk; b0 += 1024) {
        const int64_t v = b0 + tid < nblk ? wk.blk[b0 + tid] : 0;
        int64_t x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(x, o, 64);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        int64_t base = 0, tot = 0;
        for (uint32_t i = 0; i < 16; i++) {
            base += i < wv ? s_w[i] : 0;
            tot += s_w[i];
        }
        if (b0 + tid < nblk) wk.blk[b0 + tid] = carry + base + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t leave = wk.st[geo.ntiles];
        const uint64_t total = (uint64_t)(carry - (int64_t)hh_state_delta(leave));
        wk.flags[2] = (uint32_t)total;
        wk.flags[3] = (uint32_t)(total >> 32);
        wk.flags[14] = leave;
        wk.flags[15] = geo.emit_from < geo.ntiles ? wk.st[geo.emit_from] : geo.in_state;
    }
}

// ---------------------------------------------------------------------------
// The emission loops take whole L1 lookups while p < this bound, then one
// lookup or symbol at a time.  A run's symbols all end by its end pe (a
// boundary of the true chain): a lookup from p < pe - HH_P ends by pe, and so
// does an escape's single symbol.  Only the stream's last run, which may end
// in a code cut by the end of the stream (the tail rule), keeps the longest
// code's margin.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t whole_lookups_end(uint32_t pe, uint32_t bt, uint32_t maxadv) {
    const uint32_t m = pe < bt ? HH_P : maxadv;
    return pe > m ? pe - m : 0u;
}

// ---------------------------------------------------------------------------
// A run [cu.p, pe) of the true chain decoded straight to HBM at dst: bytes up
// to a dword boundary, then dwords, then the ragged end (the first and last
// dwords may be shared with the neighbouring runs).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void emit_run_direct(const hh_ctx *c, hh_cur cu, uint32_t pe, uint8_t *dst,
                                                uint32_t maxadv) {
    uint32_t o = 0, val, k;
    while ((((uintptr_t)dst + o) & 3u) && cu.p < pe) {
        const uint32_t ha = o + (4u - (uint32_t)(((uintptr_t)dst + o) & 3u));
        hh_emit_step(c, cu, pe, o, ha, &val, &k);
        for (uint32_t i = 0; i < k; i++) dst[o + i] = (uint8_t)(val >> (8 * i));
        o += k;
    }
    uint64_t acc = 0;
    uint32_t nacc = 0;
    const uint32_t pf_end = whole_lookups_end(pe, c->bt, maxadv);
    while (cu.p < pf_end) {
        const uint32_t win = hh_cur_win(cu);
        const uint64_t le = c->l1[win & (HH_L1_SIZE - 1u)];
        const uint32_t m = (uint32_t)(le >> 32);
        uint32_t sy = (uint32_t)le, ns = HH_M_NSYM(m), nb = HH_M_NBITS(m);
        if (ns == 0) {
            nb = hh_escape(c, cu.p, win, m, &sy);
            ns = 1;
        }
        acc |= (uint64_t)sy << (8 * nacc);
        nacc += ns;
        if (nacc >= 4) {
            *(uint32_t *)(dst + o) = (uint32_t)acc;
            acc >>= 32;
            nacc -= 4;
            o += 4;
        }
        hh_cur_adv(c, cu, nb);
    }
    while (cu.p < pe) {
        hh_emit_step(c, cu, pe, o + nacc, ~0ull, &val, &k);
        acc |= (uint64_t)val << (8 * nacc);
        nacc += k;
        if (nacc >= 4) {
            *(uint32_t *)(dst + o) = (uint32_t)acc;
            acc >>= 32;
            nacc -= 4;
            o += 4;
        }
    }
    for (uint32_t i = 0; i < nacc; i++) dst[o + i] = (uint8_t)(acc >> (8 * i));
}

// ---------------------------------------------------------------------------
// k_emit: pass 2 of every emitted tile, one tile per wave at a time (wave gw
// takes tiles f0 + gw, f0 + gw + #waves, ...; f0 = emit_from).  Like
// k_front, a wave never waits for another: its tile's words, live lanes,
// run offsets (a wave scan) and output staging are its own.
// ---------------------------------------------------------------------------
template <uint32_t SW, uint32_t NW>
__global__ __launch_bounds__(64 * NW) void k_emit(const uint32_t *__restrict__ gdata, Geometry geo,
                                                               DevTab tab, Work wk, uint8_t *__restrict__ out,
                                                               uint64_t cap, uint64_t *dbg) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr uint32_t NL = 64 * NW;
    __shared__ uint16_t s_eina[NW][HH_NR];  // run entries pushed by walkers
    __shared__ int16_t s_dina[NW][HH_NR];   // their deltas
    __shared__ uint8_t s_ka[NW][HH_NR];
    __shared__ uint8_t s_mema[NW][HH_NR];

    constexpr uint32_t S = 32 * SW;
    const uint32_t j = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t *s_l1 = (uint64_t *)smem;                  // L1 entries as in global memory: one
                                                        // 64-bit read gives meta and symbols
    uint32_t *s_out = (uint32_t *)(s_l1 + HH_L1_SIZE) + wv * (HH_OBW / 4);   // the wave's staging
    uint32_t *s_w = (uint32_t *)(s_l1 + HH_L1_SIZE) + NW * (HH_OBW / 4) + wv * (SW * HH_NLS);
    uint32_t *s_l2 = (uint32_t *)(s_l1 + HH_L1_SIZE) + NW * (HH_OBW / 4 + SW * HH_NLS);
    uint32_t *s_tree = s_l2 + tab.l2_used;              // the compact tree (tail rule, long codes)
    uint8_t *s_tsym = (uint8_t *)(s_tree + tab.tree_lds);
    uint16_t *s_ein = s_eina[wv];
    int16_t *s_din = s_dina[wv];

    const uint64_t tile_bits = (uint64_t)HH_NR * S;
    const uint32_t span = HH_NCOL * S;
    for (uint32_t i = threadIdx.x; i < HH_L1_SIZE; i += NL) s_l1[i] = tab.l1[i];
    for (uint32_t i = threadIdx.x; i < tab.l2_used; i += NL) s_l2[i] = tab.l2[i];
    // with the tree in LDS too, the decode loops issue no global load: a
    // global load there would make them wait for the next tile's prefetch
    for (uint32_t i = threadIdx.x; i < tab.tree_lds; i += NL) {
        s_tree[i] = tab.tree[i];
        s_tsym[i] = tab.tsym[i];
    }
    __syncthreads();                                    // (the only workgroup barrier)

    hh_ctx c;
    c.w = s_w;
    c.sw = SW;
    c.nls = HH_NLS;
    c.magic = 0;
    c.l1 = s_l1;
    c.l1m = nullptr;
    c.l1s = nullptr;
    c.l2 = s_l2;
    c.tree = s_tree;                                    // (fast_path_ok: the tree fits)
    c.tsym = s_tsym;
    c.maxadv = geo.maxadv;
    c.G = geo.G;

    // The next tile's words, lane record, entering state and output base are
    // loaded one tile ahead (they are the loads every phase below waits on),
    // the meta words BEFORE the words (vmcnt retires in order: consuming them
    // then does not wait for the words).  The entering state and base are
    // uniform, but a uniform load is moved to an SGPR -- and waited for -- at
    // once; so lanes 0..3 load one word each (state, base low, base high,
    // block-local prefix), read out of those lanes where consumed.  Loads run
    // unconditionally, past the last tile on the last tile again.
    const uint64_t f0 = geo.emit_from;
    const uint64_t nwv = (uint64_t)gridDim.x * NW;
    const uint64_t tlast = geo.ntiles - 1;              // (launched only when f0 < ntiles)
    auto clampt = [&](uint64_t tt) { return tt < tlast ? tt : tlast; };
    Prefetch pf;
    uint32_t rec_n = 0, meta_n = 0;
    auto prefetch_next = [&](uint64_t tt) {
        rec_n = wk.recs[tt * HH_NR + j];
        const uint32_t *blk32 = (const uint32_t *)wk.blk + 2 * (tt / HH_SCAN_TB);
        const uint32_t ln = j & 3u;
        const uint32_t *src = ln == 0 ? &wk.st[tt] : ln == 1 ? blk32 : ln == 2 ? blk32 + 1
                                                                   : (const uint32_t *)&wk.lex[tt];
        meta_n = *src;
        prefetch_wtile<SW>(pf, gdata, tt * tile_bits / 32, geo.nwords);
    };
    uint64_t t = f0 + (uint64_t)blockIdx.x * NW + wv;
    const uint32_t gwe = blockIdx.x * NW + wv;       // this wave's list of deferred runs
    uint32_t xqn = 0;
    if (t < geo.ntiles) prefetch_next(t);
    EDIAG_DECL
    for (; t < geo.ntiles; t += nwv) {
        WAVE_SYNC();                                    // the previous tile's LDS no longer read
        const uint64_t rem = geo.bits - t * tile_bits;
        c.bt = rem < span ? (uint32_t)rem : span;
        const uint32_t bt = c.bt;
        store_wtile<SW>(pf, s_w);
        const uint32_t rec = rec_n;
        // (readlane returns int: every word is cast to uint32_t before widening)
        const uint32_t st_in = (uint32_t)__builtin_amdgcn_readlane(meta_n, 0);
        const uint32_t blo = (uint32_t)__builtin_amdgcn_readlane(meta_n, 1);
        const uint32_t bhi = (uint32_t)__builtin_amdgcn_readlane(meta_n, 2);
        const int32_t lex_t = __builtin_amdgcn_readlane(meta_n, 3);
        const int64_t base_t = (int64_t)(((uint64_t)bhi << 32) | blo) + (int64_t)lex_t;
        prefetch_next(clampt(t + nwv));
        const uint32_t kk = rec_k(rec), ee = rec_e(rec);
        const int32_t dl = rec_delta(rec);
        const uint32_t mem = resolve_live_wave(kk, s_ka[wv], s_mema[wv]);

        // the entering state: first live lane d_t, entered e_t bits in
        const uint32_t d_t = hh_state_d(st_in);
        const int32_t dprev = hh_state_delta(st_in);
        const bool live = (mem >> d_t) & 1u;
        if (live && j + kk < HH_NR) {
            s_ein[j + kk] = (j + kk) * S + ee;
            s_din[j + kk] = (int16_t)dl;
        }
        WAVE_SYNC();
        const uint32_t e_in = j == d_t ? d_t * S + hh_state_e(st_in) : s_ein[j];
        const int32_t d_in = j == d_t ? dprev : (int32_t)s_din[j];
        const uint32_t rc = live ? (uint32_t)((int32_t)rec_nc(rec) + d_in) : 0u;
        const int32_t incl = wave_incl_scan((int32_t)rc);
        const uint32_t L = (uint32_t)incl - rc;
        const uint32_t Tout = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
        const int64_t P0s = base_t - (int64_t)dprev;
        const uint64_t P0 = (uint64_t)P0s;
        // the tile's output fits [0, cap) (no wrap-around)
        const bool fits = P0s >= 0 && P0 <= cap && Tout <= cap - P0;
        if (j == 0 && !fits) atomicOr(wk.flags, (uint32_t)F_OVER);

        hh_cur cu = hh_cur_at(&c, live ? e_in : 0u);
        const uint32_t y = (j + kk) * S + ee;
        uint32_t pe = (live && fits) ? (y < bt ? y : bt) : 0u;
        {
            // A run over several regions (a walk that crossed them) would hold
            // up the wave for as many regions: it goes to the wave's list for
            // k_emitx (lane-parallel), unless the list is full.  Its bytes
            // are copied out as zeros here and written by k_emitx after.
            const bool want = kk > 1 && cu.p < pe;
            const uint64_t dm = __ballot(want);
            const uint32_t nd = (uint32_t)__builtin_popcountll(dm);
            if (nd && xqn + nd <= geo.xcap) {
                if (want) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
                    uint64_t *xe = wk.xq + 2 * ((uint64_t)gwe * geo.xcap + xqn + rank);
                    xe[0] = P0 + L;
                    xe[1] = (t << 32) | cu.p | (pe << 16);
                    pe = 0;
                }
                xqn += nd;
            }
        }
        // The tile's output [P0, P0 + Tout) is staged in the wave's LDS at
        // byte a0 = P0 mod 16, so that 16-B blocks of LDS and of HBM line
        // up: lanes OR their symbols in as dwords (a dword two runs share
        // needs the OR; the buffer is zeroed first), then the wave copies it
        // out with whole 16-B stores -- every line written once.
        const uint32_t a0 = (uint32_t)(P0 & 15u);
        if (fits && a0 + Tout <= HH_OBW) {
            EDIAG_STAMP(0);                             // (records, live lanes, scan)
            const uint32_t nq = (a0 + Tout + 15u) / 16u;
            for (uint32_t i = j; i < nq; i += 64) *(u32x4 *)(s_out + 4 * i) = (u32x4){0u, 0u, 0u, 0u};
            WAVE_SYNC();
            EDIAG_STAMP(1);                             // (zeroing)
            if (cu.p < pe) {
                const uint32_t b = a0 + L;
                uint32_t wd = b >> 2, nacc = b & 3u, val, k;
                uint64_t acc = 0;
                const uint32_t pf_end = whole_lookups_end(pe, bt, geo.maxadv);
                while (cu.p < pf_end) {            // whole lookups
                    const uint32_t win = hh_cur_win(cu);
                    const uint32_t ix = win & (HH_L1_SIZE - 1u);
                    const uint64_t le = s_l1[ix];
                    const uint32_t m = (uint32_t)(le >> 32);
                    uint32_t sy = (uint32_t)le, ns = HH_M_NSYM(m), nb = HH_M_NBITS(m);
                    if (ns == 0) {
                        nb = hh_escape(&c, cu.p, win, m, &sy);
                        ns = 1;
                    }
                    acc |= (uint64_t)sy << (8 * nacc);
                    nacc += ns;
                    if (nacc >= 4) {
                        atomicOr(&s_out[wd], (uint32_t)acc);
                        wd++;
                        acc >>= 32;
                        nacc -= 4;
                    }
                    hh_cur_adv(&c, cu, nb);
                }
                uint32_t emitted = 4 * wd + nacc - b;
                while (cu.p < pe) {                // the end of the run (and of the stream)
                    hh_emit_step(&c, cu, pe, emitted, rc, &val, &k);
                    acc |= (uint64_t)val << (8 * nacc);
                    nacc += k;
                    emitted += k;
                    if (nacc >= 4) {
                        atomicOr(&s_out[wd], (uint32_t)acc);
                        wd++;
                        acc >>= 32;
                        nacc -= 4;
                    }
                }
                if (nacc) atomicOr(&s_out[wd], (uint32_t)acc);
            }
            EDIAG_STAMP(2);                             // (own decode)
            WAVE_SYNC();
            uint8_t *gb = out + (P0 - a0);
            const uint8_t *sb = (const uint8_t *)s_out;
            for (uint32_t i = j; i < nq; i += 64) {
                const uint32_t lo = 16 * i;
                if (lo >= a0 && lo + 16 <= a0 + Tout) {
                    __builtin_nontemporal_store(*(const u32x4 *)(sb + lo), (u32x4 *)(gb + lo));
                } else {                           // a block shared with a neighbouring tile
                    const uint32_t e = lo + 16 < a0 + Tout ? lo + 16 : a0 + Tout;
                    for (uint32_t q = lo > a0 ? lo : a0; q < e; q++) gb[q] = sb[q];
                }
            }
            EDIAG_STAMP(4);                             // (copy-out)
            continue;
        }
        // a tile too large for the staging buffer: this lane's symbols
        // straight to HBM (output bytes [P0 + L, P0 + L + rc))
        if (cu.p < pe) emit_run_direct(&c, cu, pe, out + P0 + L, geo.maxadv);
    }
    if (j == 0) wk.xqn[gwe] = xqn;
    EDIAG_FLUSH(dbg);
}

// ---------------------------------------------------------------------------
// k_emitx: the runs k_emit deferred (several regions long), one lane each,
// over the lane's own staging of the run's words at LDS index
// (g - g0) * 64 + lane; straight to HBM (emit_run_direct).
// ---------------------------------------------------------------------------
template <uint32_t SW>
struct EmitxWin {
    static constexpr uint32_t n = (HH_KM + 1) * SW + 6;
};

template <uint32_t SW>
__global__ __launch_bounds__(64) void k_emitx(const uint32_t *__restrict__ gdata, Geometry geo, DevTab tab, Work wk,
                                              uint8_t *__restrict__ out, uint32_t nwe) {
    extern __shared__ __align__(16) uint8_t smem[];
    constexpr uint32_t S = 32 * SW, NW = EmitxWin<SW>::n;
    const uint32_t lane = threadIdx.x;
    uint64_t *s_l1 = (uint64_t *)smem;
    uint32_t *s_l2 = (uint32_t *)(s_l1 + HH_L1_SIZE);
    uint32_t *s_win = s_l2 + ((tab.l2_used + 3u) & ~3u) + lane;   // NW x 64 words
    for (uint32_t i = lane; i < HH_L1_SIZE; i += 64) s_l1[i] = tab.l1[i];
    for (uint32_t i = lane; i < tab.l2_used; i += 64) s_l2[i] = tab.l2[i];
    __syncthreads();
    const uint64_t tile_bits = (uint64_t)HH_NR * S;
    const uint32_t span = HH_NCOL * S;
    hh_ctx c;
    c.sw = 1024;                                        // hh_idx(g) = g * 64 (below)
    c.nls = 64;
    c.magic = 0;
    c.l1m = nullptr;
    c.l1s = nullptr;
    c.l1 = s_l1;
    c.l2 = s_l2;
    c.tree = tab.tree;
    c.tsym = tab.tsym;
    c.maxadv = geo.maxadv;
    c.G = geo.G;
    uint32_t fw = blockIdx.x, i = lane, cnt = fw < nwe ? wk.xqn[fw] : 0u;
    for (;;) {
        while (i >= cnt && fw < nwe) {
            i -= cnt;
            fw += gridDim.x;
            cnt = fw < nwe ? wk.xqn[fw] : 0u;
        }
        if (fw >= nwe) break;
        const uint64_t *xe = wk.xq + 2 * ((uint64_t)fw * geo.xcap + i);
        i += 64;
        const uint64_t O = xe[0], w1 = xe[1];
        const uint64_t t = w1 >> 32;
        const uint32_t e_in = (uint32_t)w1 & 0xffffu, pe = ((uint32_t)w1 >> 16) & 0xffffu;
        const uint64_t rem = geo.bits - t * tile_bits;
        c.bt = rem < span ? (uint32_t)rem : span;
        const uint32_t g0 = e_in >> 5;
        const uint64_t gw0 = t * tile_bits / 32 + g0, glim = geo.nwords;
#pragma unroll 8
        for (uint32_t q = 0; q < NW; q++) {
            const uint64_t gi = gw0 + q;
            s_win[q * 64] = gdata[gi < glim ? gi : glim - 1];
        }
        c.w = s_win - (int32_t)(g0 * 64);
        emit_run_direct(&c, hh_cur_at(&c, e_in), pe, out + O, geo.maxadv);
    }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
typedef void (*kfront_t)(const uint32_t *, Geometry, DevTab, Work, uint64_t *);
typedef void (*kemit_t)(const uint32_t *, Geometry, DevTab, Work, uint8_t *, uint64_t, uint64_t *);

static size_t lds_front(uint32_t sw, uint32_t l2, uint32_t fdir) {
    return ((size_t)ftab_words(fdir, l2) + (size_t)HH_FW * sw * HH_NLS) * 4;
}
static uint32_t walk_win(uint32_t sw) { return sw + 6; }   // WalkWin<sw>::n
static size_t lds_walk(uint32_t sw, uint32_t l2, uint32_t fdir) {
    return ((size_t)ftab_words(fdir, l2) + (size_t)walk_win(sw) * HH_WALK_T) * 4;
}
static size_t lds_emitx(uint32_t sw, uint32_t l2) {
    return (size_t)HH_L1_SIZE * 8 + (size_t)((l2 + 3) & ~3u) * 4 + (size_t)((HH_KM + 1) * sw + 6) * 64 * 4;
}
static size_t lds_emit(uint32_t sw, uint32_t l2, uint32_t tree, uint32_t nw) {
    return (2 * (size_t)HH_L1_SIZE + (size_t)nw * sw * HH_NLS + l2) * 4 + (size_t)nw * HH_OBW +
           (size_t)tree * 5;
}

// kernels instantiated per words-per-region (S = 32 * SW bits)
#define HH_SW_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
static kfront_t kfront_for(uint32_t sw) {
    switch (sw) {
#define X(n) case n: return k_front<n>;
        HH_SW_CASES(X)
#undef X
    default: return nullptr;
    }
}
typedef void (*kwalk_t)(const uint32_t *, Geometry, DevTab, Work);
static kwalk_t kwalk_for(uint32_t sw) {
    switch (sw) {
#define X(n) case n: return k_walk<n>;
        HH_SW_CASES(X)
#undef X
    default: return nullptr;
    }
}
typedef void (*kemitx_t)(const uint32_t *, Geometry, DevTab, Work, uint8_t *, uint32_t);
static kemitx_t kemitx_for(uint32_t sw) {
    switch (sw) {
#define X(n) case n: return k_emitx<n>;
        HH_SW_CASES(X)
#undef X
    default: return nullptr;
    }
}
static kemit_t kemit_for(uint32_t sw, uint32_t nw) {
    switch (sw) {
#define X(n) case n: return nw == 16 ? k_emit<n, 16> : k_emit<n, 8>;
        HH_SW_CASES(X)
#undef X
    default: return nullptr;
    }
}

// Persistent grids: the occupancy answer x CUs for each kernel.
static int size_grids(hh_decoder *d, uint32_t sw) {
    if (d->grid_f && d->grid_sw == sw && d->grid_l2 == d->tab.l2_used && d->grid_tree == d->tab.tree_lds &&
        d->grid_fdir == d->tab.fdir_used && d->grid_nw_max == d->emit_nw_max)
        return HH_OK;
    int pf = 0, pe = 0, pw = 0, px = 0, ncu = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pf, kfront_for(sw), 64 * HH_FW, lds_front(sw, d->tab.l2_used, d->tab.fdir_used)));
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pw, kwalk_for(sw), HH_WALK_T, lds_walk(sw, d->tab.l2_used, d->tab.fdir_used)));
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&px, kemitx_for(sw), 64, lds_emitx(sw, d->tab.l2_used)));
    uint32_t nw = d->emit_nw_max;
    for (;; nw /= 2) {
        pe = 0;
        const size_t lds = lds_emit(sw, d->tab.l2_used, d->tab.tree_lds, nw);
        if (lds + (size_t)nw * HH_NR * 6 <= 160 * 1024)   // (+ the static per-wave arrays)
            HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&pe, kemit_for(sw, nw), 64 * nw, lds));
        if (pe >= 1 || nw == 8) break;
    }
    d->emit_nw = nw;
    HIP_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, d->device));
    if (pf < 1 || pe < 1 || pw < 1 || px < 1) return HH_ERR_UNSUPPORTED;
    d->grid_f = (uint32_t)(pf * ncu);
    d->grid_w = (uint32_t)(pw * ncu);
    d->grid_x = (uint32_t)(px * ncu);
    d->ncu = (uint32_t)ncu;
    d->grid_e = (uint32_t)(pe * ncu);
    d->grid_sw = sw;
    d->grid_l2 = d->tab.l2_used;
    d->grid_tree = d->tab.tree_lds;
    d->grid_fdir = d->tab.fdir_used;
    d->grid_nw_max = d->emit_nw_max;
    return HH_OK;
}

// The host's version of k_scan1/k_scan2 for streams whose non-CONST chains
// are longer than HH_SCAN_BACK tiles (codes that resynchronise but whose
// leaving state stays entry-dependent for thousands of tiles): one
// sequential pass over the tables.
static int scan_host(hh_decoder *d, const Geometry &geo, const Work &wk, uint32_t nblk, hipStream_t st) {
    const uint64_t nt = geo.ntiles;
    uint64_t *tabs = (uint64_t *)malloc(nt * HH_KM * 8);
    uint32_t *sts = (uint32_t *)malloc((nt + 1) * 4);
    int32_t *lex = (int32_t *)malloc((nt + 1) * 4);
    int64_t *blk = (int64_t *)malloc((size_t)nblk * 8);
    int rc = HH_OK;
    if (!tabs || !sts || !lex || !blk) { rc = HH_ERR_NOMEM; goto out; }
    if (hipMemcpyAsync(tabs, wk.tabs, nt * HH_KM * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { rc = HH_ERR_DEVICE; goto out; }
    {
        uint32_t s = geo.in_state;
        int64_t run = geo.emit_from ? 0 : hh_state_delta(geo.in_state), bsum = 0;
        for (uint64_t t = 0; t <= nt; t++) {
            if (t % HH_SCAN_TB == 0) {
                blk[t / HH_SCAN_TB] = run;
                bsum = 0;
            }
            sts[t] = s;
            lex[t] = (int32_t)bsum;
            if (t == nt) break;
            const uint64_t row = tabs[t * HH_KM + (hh_state_d(s) & (HH_KM - 1u))];
            int32_t cnt = hh_tab_count(row);
            if (t < geo.emit_from) cnt = t + 1 == geo.emit_from ? hh_state_delta(hh_tab_state(row)) : 0;
            bsum += cnt;
            run += cnt;
            s = hh_tab_state(row);
        }
        const uint64_t total = (uint64_t)(run - hh_state_delta(s));
        uint32_t fl[16];
        memcpy(fl, d->h_flags, sizeof(fl));
        fl[0] &= ~(uint32_t)F_SCAN;
        fl[2] = (uint32_t)total;
        fl[3] = (uint32_t)(total >> 32);
        fl[14] = s;
        fl[15] = geo.emit_from < nt ? sts[geo.emit_from] : geo.in_state;
        if (hipMemcpyAsync(wk.st, sts, (nt + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(wk.lex, lex, (nt + 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(wk.blk, blk, (size_t)nblk * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(wk.flags, fl, sizeof(fl), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            rc = HH_ERR_DEVICE;
    }
out:
    free(tabs);
    free(sts);
    free(lex);
    free(blk);
    return rc;
}

// The fused decode of tiles [0, ntiles) of the segment at d_data
// (bits_avail readable stream bits), entered at in_state.
int decode_fast(hh_decoder *d, const void *d_data, uint64_t bits_avail, uint64_t ntiles,
                uint32_t in_state, uint64_t emit_from, void *d_out, uint64_t cap,
                hipStream_t st, uint64_t *total, uint32_t *leave, uint32_t *cst_pro,
                uint32_t *cst_seg, uint32_t *entry) {
    Geometry geo;
    geo.bits = bits_avail;
    geo.S = d->S;
    geo.sw = d->S / 32;
    geo.maxadv = d->ht->maxlen > HH_P ? (uint32_t)d->ht->maxlen : HH_P;
    geo.G = d->G;
    geo.nwords = ((bits_avail + 7) / 8 + HH_PAYLOAD_PAD) / 4;
    geo.in_state = in_state;
    geo.emit_from = emit_from;
    geo.fwalk = d->fwalk;
    const uint64_t tb = (uint64_t)HH_NR * d->S;
    const uint64_t all = (bits_avail + tb - 1) / tb;
    geo.ntiles = ntiles && ntiles < all ? ntiles : all;
    const uint64_t nt = geo.ntiles;
    const uint32_t nblk = (uint32_t)((nt + 1 + HH_SCAN_TB - 1) / HH_SCAN_TB);
    // workspace: flags 64 B | tabs | recs | st | lex | blk | q
    const size_t o_tabs = 64, o_recs = o_tabs + nt * HH_KM * 8, o_st = o_recs + nt * HH_NR * 4;
    const size_t o_lex = (o_st + (nt + 1) * 4 + 7) & ~(size_t)7, o_blk = (o_lex + (nt + 1) * 4 + 7) & ~(size_t)7;
    int rc = size_grids(d, geo.sw);
    if (rc) return rc;
    // one tile per wave at a time in both kernels
    const uint64_t nfw = (nt + HH_FW - 1) / HH_FW;
    const uint32_t gf = (uint32_t)(nfw < d->grid_f ? nfw : d->grid_f);
    geo.nfw = gf * HH_FW;
    geo.qcap = (nt + geo.nfw - 1) / geo.nfw * HH_NR;
    const size_t o_qn = o_blk + (size_t)nblk * 8, o_q = (o_qn + (size_t)geo.nfw * 4 + 7) & ~(size_t)7;
    const size_t o_xn = o_q + (size_t)geo.nfw * geo.qcap * 8;
    const uint64_t ne = nt > emit_from ? nt - emit_from : 0;
    const uint32_t enw = d->emit_nw;
    const uint64_t ng = (ne + enw - 1) / enw;              // workgroups' worth of tiles
    const uint32_t ge = (uint32_t)(ng < d->grid_e ? (ng ? ng : 1) : d->grid_e);
    const uint32_t nwe = ge * enw;                          // k_emit's waves
    geo.xcap = (uint32_t)((ne + nwe - 1) / nwe * d->xpt);
    const size_t o_xqn = o_xn + (nt + 1) * HH_NR * 4, o_xq = (o_xqn + (size_t)nwe * 4 + 15) & ~(size_t)15;
    const size_t need = o_xq + (size_t)nwe * geo.xcap * 16;
    rc = ensure_dev(&d->ws, &d->ws_size, need);
    if (rc) return rc;
    uint8_t *w = (uint8_t *)d->ws;
    Work wk;
    wk.flags = (uint32_t *)w;
    wk.tabs = (uint64_t *)(w + o_tabs);
    wk.recs = (uint32_t *)(w + o_recs);
    wk.st = (uint32_t *)(w + o_st);
    wk.lex = (int32_t *)(w + o_lex);
    wk.blk = (int64_t *)(w + o_blk);
    wk.q = (uint64_t *)(w + o_q);
    wk.qn = (uint32_t *)(w + o_qn);
    wk.xn = (uint32_t *)(w + o_xn);
    wk.xqn = (uint32_t *)(w + o_xqn);
    wk.xq = (uint64_t *)(w + o_xq);
    const kfront_t kf = kfront_for(geo.sw);
    const kwalk_t kw = kwalk_for(geo.sw);
    const kemit_t ke = kemit_for(geo.sw, enw);
    const kemitx_t kx = kemitx_for(geo.sw);
    if (!kf || !kw || !ke || !kx) return HH_ERR_UNSUPPORTED;
    // k_emit, then the runs it deferred
    auto launch_emit = [&]() -> int {
        hipLaunchKernelGGL(ke, dim3(ge), dim3(64 * enw), lds_emit(geo.sw, d->tab.l2_used, d->tab.tree_lds, enw), st,
                           (const uint32_t *)d_data, geo, d->tab, wk, (uint8_t *)d_out, cap, d->d_dbg);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(kx, dim3(d->grid_x), dim3(64), lds_emitx(geo.sw, d->tab.l2_used), st,
                           (const uint32_t *)d_data, geo, d->tab, wk, (uint8_t *)d_out, nwe);
        HIP_OK(hipGetLastError());
        return HH_OK;
    };

    HIP_OK(hipMemsetAsync(wk.flags, 0, 64, st));
#ifdef HH_DIAG
    HIP_OK(hipMemsetAsync(d->d_dbg, 0, 16 * sizeof(uint64_t), st));
#endif
    HIP_OK(hipEventRecord(d->ev[0], st));
    hipLaunchKernelGGL(kf, dim3(gf), dim3(64 * HH_FW), lds_front(geo.sw, d->tab.l2_used, d->tab.fdir_used), st,
                       (const uint32_t *)d_data, geo, d->tab, wk, d->d_dbg);
    HIP_OK(hipGetLastError());
    // the deferred walks (their count is on the device: a persistent grid)
    hipLaunchKernelGGL(kw, dim3(d->grid_w), dim3(HH_WALK_T), lds_walk(geo.sw, d->tab.l2_used, d->tab.fdir_used), st,
                       (const uint32_t *)d_data, geo, d->tab, wk);
    HIP_OK(hipGetLastError());
    {
        // persistent: each wave's next record is loaded a tile ahead
        const uint64_t nb = (nt + HH_TABLE_W - 1) / HH_TABLE_W, cap = (uint64_t)d->ncu * 8;
        hipLaunchKernelGGL(k_table, dim3((unsigned)(nb < cap ? nb : cap)), dim3(64 * HH_TABLE_W), 0, st, geo, wk);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(d->ev[1], st));
    hipLaunchKernelGGL(k_scan1, dim3(nblk), dim3(HH_SCAN_TB), 0, st, geo, wk);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_scan2, dim3(1), dim3(1024), 0, st, geo, wk, nblk);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(d->ev[2], st));
    if (ne && (rc = launch_emit())) return rc;
    HIP_OK(hipEventRecord(d->ev[3], st));
    HIP_OK(hipMemcpyAsync(d->h_flags, wk.flags, 64, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if ((d->h_flags[0] & F_SCAN) && !(d->h_flags[0] & F_FAIL)) {
        // a non-CONST chain too long for k_scan1: compose on the host, emit again
        rc = scan_host(d, geo, wk, nblk, st);
        if (rc) return rc;
        if (ne && (rc = launch_emit())) return rc;
        HIP_OK(hipEventRecord(d->ev[3], st));
        HIP_OK(hipMemcpyAsync(d->h_flags, wk.flags, 64, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        d->stats.repairs++;
    }
    const uint32_t fl = d->h_flags[0];
    *total = (uint64_t)d->h_flags[2] | ((uint64_t)d->h_flags[3] << 32);
    *leave = d->h_flags[14];
    *cst_pro = d->h_flags[12];
    *cst_seg = d->h_flags[13];
    *entry = d->h_flags[15];
    if (emit_from >= nt) *total = 0;
    float ms[3] = {0, 0, 0};
    hipEventElapsedTime(&ms[0], d->ev[0], d->ev[1]);
    hipEventElapsedTime(&ms[1], d->ev[1], d->ev[2]);
    hipEventElapsedTime(&ms[2], d->ev[2], d->ev[3]);
    d->stats.ms_sync = ms[0];
    d->stats.ms_scan = ms[1];
    d->stats.ms_emit = ms[2];
    d->stats.ms_total = ms[0] + ms[1] + ms[2];
    d->stats.lanes = nt * HH_NR;
    d->stats.out_len = *total;
    if (fl & F_FAIL) return HH_NOSYNC;
    if (*total > cap || (fl & F_OVER)) return HH_ERR_CAPACITY;
    return HH_OK;
}

// Diagnostic: the first failed walk of the last decode (tile, lane, exit,
// count, tile end); 0 if none.
extern "C" int hh_debug_failure(hh_decoder *d, uint32_t *out5) {
    if (!d || !out5 || !d->ws) return 0;
    uint32_t f[10];
    if (hipMemcpy(f, d->ws, sizeof(f), hipMemcpyDeviceToHost) != hipSuccess) return HH_ERR_DEVICE;
    for (int i = 0; i < 5; i++) out5[i] = f[5 + i];
    return (int)f[4];
}

// Diagnostic (HH_DIAG builds; zeros otherwise): the front kernel's phase
// cycles summed over workgroups [0..3] (staging, pass 1, walks, table) and
// walk statistics [8..11] (lanes, lookups, sum over waves of the wave's
// longest walk, longest walk) of the last decode; HH_DBG_WORDS words.
extern "C" int hh_debug_counters(hh_decoder *d, uint64_t *out16) {
    if (!d || !out16) return HH_ERR_ARG;
    if (hipMemcpy(out16, d->d_dbg, HH_DBG_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return HH_ERR_DEVICE;
    return HH_OK;
}
