/*
 * hh_batch_algo.h -- the rules of a round of the batched decode
 * (hh_batch.hip: k_batch), __host__ __device__: the kernel runs them per
 * lane, the test-only emulator (tests/emu/hh_batch_emu.cpp) runs the same
 * decomposition lane by lane on the host, against the oracle.
 *
 * A batch is n independent streams of one code.  A workgroup of W waves
 * decodes a stream in ROUNDS of W tiles (64 W regions of S bits, lane =
 * region), carrying the state that enters the round's first region (the
 * root for the stream's first) and the output base from round to round:
 *
 *   guess   region j > 0 of a round is entered in the state a chain started
 *           at the root G bits before it has reached (hb_guess; G =
 *           hh_fsm_pick_head over the emission step K); region 0 in the
 *           carried state, which is exact.
 *   count   a region's count and exit state from its entry (hb_region with
 *           a sink that stores nothing: an emission entry carries the
 *           number of symbols and the next state, so the count pass walks
 *           the emission tables and needs no count table).
 *   fix     a lane whose predecessor's exit differs from its own entry takes
 *           that exit as its entry and counts again (hb_fix); repeated until
 *           no lane changes.  After k fix rounds regions 0..k are right, so
 *           HB_FIX_BOUND(W) rounds always suffice: a code that never
 *           resynchronises is exact, only slow.
 *   scan    exclusive prefix sum of the counts: a region's output offset.
 *   emit    hb_region again, the sink storing the symbols; of the round's
 *           bytes [base, base + n) those below the stream's capacity are
 *           copied out (hb_clip) -- the count goes on past the capacity,
 *           out_len is the stream's full symbol count.
 *   window  a piece of a range read wants the stream's bytes [skip, skip +
 *           cap) only (hb_window): rounds before the window are counted, not
 *           emitted, and the piece ends with the round that fills the window
 *           (hb_window_done); its length is the bytes delivered.
 *
 * The stream's last region (the one `bits` ends in: hb_span's at_end) takes
 * whole K-bit steps while they fit, the rest bit by bit (b1), and the tail
 * rule of hh_fsm_algo.h: a chain that is not at the root at the end of the
 * stream adds the symbol of the node reached.
 */
#ifndef HH_BATCH_ALGO_H_
#define HH_BATCH_ALGO_H_

#include <stdint.h>

#include "hh_fsm.h"
#include "hh_fsm_algo.h"

#if defined(__HIPCC__)
#define HB_MD __host__ __device__ __forceinline__
#else
#define HB_MD inline
#endif

#define HB_NR 64                                   /* regions per tile (a wave) */
#define HB_WMAX 16                                 /* waves per workgroup, at most */
#define HB_FIX_BOUND(W) (HB_NR * (W) + 1u)         /* fix rounds incl. the one that changes nothing */

/* The emission tables of a tree (hh_fsm.h); on the device they lie in LDS. */
typedef struct {
    const uint64_t *et, *er;
    const uint32_t *b1;
    const uint8_t *tsym;
    uint32_t K, r, S;
} hb_view;

/* Stream bits from a word array, K or fewer at a time: a 64-bit buffer
 * refilled a word at a time.  Reads up to two words past the last bit taken
 * (never as stream bits). */
typedef struct {
    const uint32_t *w;
    uint64_t buf;
    uint32_t have;
} hb_bits;

HH_FD void hb_bits_init(hb_bits *b, const uint32_t *w, uint64_t p) {
    const uint32_t o = (uint32_t)(p & 31);
    b->w = w + (p >> 5) + 2;
    b->buf = ((uint64_t)b->w[-2] | (uint64_t)b->w[-1] << 32) >> o;
    b->have = 64u - o;
}
HH_FD uint32_t hb_bits_take(hb_bits *b, uint32_t n) {
    const uint32_t v = (uint32_t)b->buf & ((1u << n) - 1u);
    b->buf >>= n;
    b->have -= n;
    if (b->have <= 32u) {
        b->buf |= (uint64_t)*b->w++ << b->have;
        b->have += 32u;
    }
    return v;
}

/* Region [R, R + S) of a stream of `bits` bits: the bits it walks (0: past
 * the end, an idle lane), whether it is whole, whether the stream ends in it
 * (the lane that applies the tail rule). */
HH_FD uint32_t hb_span(uint64_t R, uint32_t S, uint64_t bits, int *whole, int *at_end) {
    *whole = R + S <= bits;
    *at_end = R < bits && R + S >= bits;
    if (R >= bits) return 0u;
    return *whole ? S : (uint32_t)(bits - R);
}

/* The guess of a region's entering state: a chain from the root over the G
 * bits before it (G a multiple of K; b at the first of them). */
HH_FD uint32_t hb_guess(const hb_view *F, hb_bits *b, uint32_t G) {
    const uint32_t lg = HH_FSM_ET_LG(F->K);
    uint32_t s = 0;
    for (uint32_t q = 0; q + F->K <= G; q += F->K)
        s = HH_FSM_ET_ROW(F->et[(s << lg) + hb_bits_take(b, F->K)]) >> (lg + 3u);
    return s;
}

/* A region of nb bits (hb_span) entered in state s, b at its first bit:
 * whole K-bit steps, then the r-bit step of a whole region or single bits,
 * then the tail rule when the stream ends in it.  Every step's entry goes
 * to sink.put(entry) (symbols in bits 0..31, 8 x their number in bits
 * 32..39: hh_fsm.h's emission entry).  Returns the exit state; *n the
 * symbols. */
template <class Sink>
HH_FD uint32_t hb_region(const hb_view *F, hb_bits *b, uint32_t nb, int whole, int at_end, uint32_t s,
                         Sink &sink, uint32_t *n) {
    const uint32_t K = F->K, lg = HH_FSM_ET_LG(K);
    uint32_t c8 = 0, left = nb;
    for (; left >= K; left -= K) {
        const uint64_t e = F->et[(s << lg) + hb_bits_take(b, K)];
        sink.put(e);
        c8 += (uint32_t)(e >> 32) & 255u;
        s = HH_FSM_ET_ROW(e) >> (lg + 3u);
    }
    if (whole && F->r) {
        const uint64_t e = F->er[(s << F->r) + hb_bits_take(b, F->r)];
        sink.put(e);
        c8 += (uint32_t)(e >> 32) & 255u;
        s = HH_FSM_ET_ROW(e) >> (lg + 3u);
        left = 0;
    }
    for (; left; left--) {
        const uint32_t v = F->b1[s * 2 + hb_bits_take(b, 1)];
        const uint32_t k = (v >> 8) & 255u;
        sink.put(HH_FSM_ET_MAKE((v >> 16) & 255u, 0u, k));
        c8 += 8u * k;
        s = v & 255u;
    }
    if (at_end && s != 0) {
        sink.put(HH_FSM_ET_MAKE(F->tsym[s], 0u, 1u));
        c8 += 8u;
    }
    *n = c8 >> 3;
    return s;
}

/* The count pass's sink. */
struct hb_no_sink {
    HB_MD void put(uint64_t) {}
};

/* A fix round's rule for one lane: region j of the round (j > 0), walking nb
 * bits, assumed entered in *ent, its predecessor left in state pred.  Returns
 * 1 when the lane must count again, from *ent = pred.  The fix rounds end
 * with the first one in which no lane returns 1. */
HH_FD int hb_fix(uint32_t j, uint32_t nb, uint32_t pred, uint32_t *ent) {
    if (j == 0 || nb == 0 || pred == *ent) return 0;
    *ent = pred;
    return 1;
}

/* Of a round's n bytes at offset base of the stream's output, those below
 * the capacity. */
HH_FD uint32_t hb_clip(uint64_t base, uint32_t n, uint64_t cap) {
    if (base >= cap) return 0u;
    return cap - base < n ? (uint32_t)(cap - base) : n;
}

/* The same for a window [skip, skip + cap) of the stream's output (a piece of
 * hh_decode_blocks_read: hh_batch_read_algo.h): how many of the round's n
 * bytes at offset base fall into it, *from the offset of the first of them
 * inside the round (0 when there is none).  No sum is formed: base + n and
 * skip + cap may lie past 2^64.  With skip = 0 it is hb_clip, *from 0. */
HH_FD uint32_t hb_window(uint64_t base, uint32_t n, uint64_t skip, uint64_t cap, uint32_t *from) {
    *from = 0;
    if (cap == 0) return 0u;
    if (base >= skip) {
        const uint64_t d = base - skip;
        if (d >= cap) return 0u;
        return cap - d < n ? (uint32_t)(cap - d) : n;
    }
    const uint64_t f = skip - base;
    if (f >= n) return 0u;
    *from = (uint32_t)f;
    return cap < n - (uint32_t)f ? (uint32_t)cap : n - (uint32_t)f;
}
/* A window piece's last round: the one after which the window is full
 * (seen = base + the round's bytes; skip + cap <= the stream's symbols). */
HH_FD int hb_window_done(uint64_t seen, uint64_t skip, uint64_t cap) { return seen >= skip && seen - skip >= cap; }

/* LDS of a workgroup of W waves beside the tables (tabb bytes): per tile the
 * payload rows (SW words + a pad word against bank conflicts when SW is
 * even) and the staging of the most symbols a tile can hold (a region: a
 * code entered before it, one per minlen bits, the tail rule's). */
HH_FD uint32_t hb_row_words(uint32_t S) { return (S / 32u) | 1u; }
HH_FD uint32_t hb_tile_syms(uint32_t S, uint32_t minlen) { return HB_NR * (S / (minlen ? minlen : 1u) + 2u); }
HH_FD uint32_t hb_pay_bytes(uint32_t S, uint32_t W) { return (HB_NR * W * hb_row_words(S) + 4u) * 4u; }
HH_FD uint32_t hb_misc_bytes(void) { return 3u * HB_WMAX * 4u + 16u; }
HH_FD uint32_t hb_stage_bytes(uint32_t S, uint32_t minlen, uint32_t W) {
    return (W * hb_tile_syms(S, minlen) + 16u + 8u + 15u) & ~15u;
}
HH_FD uint32_t hb_lds_bytes(uint32_t tabb, uint32_t S, uint32_t minlen, uint32_t W) {
    return ((tabb + hb_pay_bytes(S, W) + hb_misc_bytes() + 15u) & ~15u) + hb_stage_bytes(S, minlen, W);
}
/* The waves per workgroup (tiles per round): as many as the LDS holds, at
 * most HB_WMAX; 0: not even one. */
HH_FD uint32_t hb_pick_waves(uint32_t tabb, uint32_t S, uint32_t minlen, uint32_t lds) {
    uint32_t W = HB_WMAX;
    while (W && hb_lds_bytes(tabb, S, minlen, W) > lds) W--;
    return W;
}

#endif
