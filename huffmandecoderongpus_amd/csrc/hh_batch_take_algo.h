/*
 * hh_batch_take_algo.h -- the rules of the record take (hh_decode_batch_take;
 * hh_batch_take.hip: the plan's kernels and k_take), __host__ __device__: the
 * kernels run them per record and per lane, the test-only emulator
 * (tests/emu/hh_take_emu.cpp) runs the same functions on the host.
 *
 * A take names m records of an index (hh_batch_item rows: data_off, bits, cap
 * = the record's symbols) and gets their bytes one after another, with the
 * offsets that delimit them.
 *
 *   plan    per taken record j: its length (hbt_row_ok: 0 for an id past the
 *           index or a row that breaks a payload rule of hbp_item_ok), the
 *           saturating prefix sums of the lengths (d_out_offs), its fate
 *           (hbt_fate): an error, an empty record, or a STREAM of ceil(bits /
 *           S) regions.  The streams, in take order, are numbered through one
 *           sequence of SLOTS, a slot per region.
 *   cut     the slots are cut into equal shares of whole rounds (hbt_share);
 *           a workgroup's streams are those whose first slot lies in its
 *           share (hbt_lower finds the first of them), and it numbers slots
 *           from its own first stream: nothing is shared between workgroups.
 *   round   64 W consecutive slots, lane = slot.  The streams that start in
 *           the round leave a mark at their first slot (hbt_mark); a maximum
 *           scan over the marks gives every lane the ordinal of its stream in
 *           the round (0: the stream carried in from the round before) and
 *           that stream's first slot, hence its region q.  A lane with q == 0
 *           enters at the root, lane 0 with q > 0 in the carried state: both
 *           exact (hbt_exact).  Every other lane guesses from the row before
 *           it, its own stream's previous region, and is fixed from its
 *           predecessor's exit as in hh_batch_algo.h (hbt_fix).
 *   out     one scan over the round's counts.  Where every stream of the
 *           round has the count its index says (hbt_settle) the round's bytes
 *           are one contiguous range of the output and are copied as
 *           k_batch's; else every lane copies its own region's bytes, clipped
 *           to its record's length (hb_clip).
 */
#ifndef HH_BATCH_TAKE_ALGO_H_
#define HH_BATCH_TAKE_ALGO_H_

#include <stdint.h>

#include "hh_batch_algo.h"
#include "hh_batch_plan_algo.h"

#define HBT_TILE 1024u                 /* records per scan tile */
#define HBT_STREAM 0x7ffffffe          /* hbt_fate: the record is a stream for k_take */

/* A stream of the take, in take order.  slot0: its first slot in the global
 * sequence; j: its place in the take. */
typedef struct {
    uint64_t data_off, bits, slot0, out_off, len, j;
} hbt_desc;

HH_FD uint64_t hbt_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

/* Taken record with id r: 1 when it may be decoded (the id inside the index,
 * the row's payload rules kept); its length is then the row's cap, else 0. */
HH_FD int hbt_row_ok(uint64_t r, uint64_t nrec, uint64_t data_off, uint64_t bits, uint64_t data_bytes) {
    return r < nrec && hbp_item_ok(data_off, bits, 0u, 0u, data_bytes, 0u);
}

HH_FD uint64_t hbt_regions(uint64_t bits, uint32_t S) { return bits / S + (bits % S != 0); }

/* The fate of a taken record: ok from hbt_row_ok, its bits and length, end =
 * d_out_offs[j + 1].  A status, or HBT_STREAM: k_take decodes it.  A record
 * whose bits and length cannot agree needs no decode: a stream of no bits
 * holds no symbol, any other holds at least one. */
HH_FD int32_t hbt_fate(int ok, uint64_t bits, uint64_t len, uint64_t end, uint64_t out_bytes) {
    if (!ok) return HH_ERR_ARG;
    if (end > out_bytes) return HH_ERR_CAPACITY;
    if (bits == 0) return len == 0 ? HH_OK : HH_ERR_FORMAT;
    if (len == 0) return HH_ERR_FORMAT;
    return HBT_STREAM;
}

/* The slots of a workgroup's share: nslots cut into grid shares of whole
 * rounds of NL slots (forced != 0: a test's share, rounded up to rounds). */
HH_FD uint64_t hbt_share(uint64_t nslots, uint32_t grid, uint32_t NL, uint64_t forced) {
    uint64_t s = forced ? forced : nslots / grid + (nslots % grid != 0);
    uint64_t rounds = s / NL + (s % NL != 0);
    if (rounds > ~0ull / NL) rounds = ~0ull / NL;          /* (slots near 2^64: never) */
    return rounds ? rounds * NL : NL;
}

/* The first of ns streams whose first slot is at or after target (ns: none). */
HH_FD uint32_t hbt_lower(const hbt_desc *d, uint32_t ns, uint64_t target) {
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (d[mid].slot0 < target) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
/* Share edge e of a grid: the first stream of workgroup e (of none: ns). */
HH_FD uint32_t hbt_edge(const hbt_desc *d, uint32_t ns, uint64_t nslots, uint64_t share, uint32_t e) {
    const uint64_t t = (uint64_t)e * share;
    return t >= nslots ? ns : hbt_lower(d, ns, t);
}

/* A mark: the ordinal (1 ..) of a stream that starts in the round, and the
 * slot it starts at; ordered by ordinal, so the maximum scan carries the
 * last start at or before a lane.  0: no stream starts here. */
#define HBT_POS_BITS 10u               /* 64 HB_WMAX slots */
HH_FD uint32_t hbt_mark(uint32_t ord, uint32_t pos) { return ord << HBT_POS_BITS | pos; }
HH_FD uint32_t hbt_mark_ord(uint32_t m) { return m >> HBT_POS_BITS; }
HH_FD uint32_t hbt_mark_pos(uint32_t m) { return m & ((1u << HBT_POS_BITS) - 1u); }

/* Lane jr of a round whose scanned mark is m: its region in its stream.  cq:
 * the regions of the carried stream walked in earlier rounds. */
HH_FD uint64_t hbt_region_of(uint32_t jr, uint32_t m, uint64_t cq) {
    return hbt_mark_ord(m) ? (uint64_t)(jr - hbt_mark_pos(m)) : cq + jr;
}

/* A lane whose entry is exact: the root for a stream's region 0, the carried
 * state for the round's lane 0. */
HH_FD int hbt_exact(uint32_t jr, uint64_t q) { return jr == 0 || q == 0; }
HH_FD uint32_t hbt_entry(uint64_t q, uint32_t carry) { return q == 0 ? 0u : carry; }
HH_FD int hbt_fix(int exact, uint32_t nb, uint32_t pred, uint32_t *ent) {
    return exact ? 0 : hb_fix(1u, nb, pred, ent);
}

/* A stream after a round: before symbols in earlier rounds, n in this one,
 * ended: its last region was in the round.  Returns 0 when the round may be
 * copied out as one range -- the stream has the count its index says, or may
 * still come to it; *status: the ended stream's. */
HH_FD int hbt_settle(uint64_t before, uint32_t n, uint64_t len, int ended, int32_t *status) {
    const uint64_t c = before + n;
    *status = c == len ? HH_OK : HH_ERR_FORMAT;
    return ended ? c != len : c > len;
}
/* A stream that starts in the round at the round's byte `first` lies in that
 * one range when its output offset is the range's (ga: the offset of the
 * round's byte 0).  Not so after a record that holds bytes of the output and
 * is no stream (over the capacity, or bits == 0 with a length). */
HH_FD int hbt_in_place(uint64_t ga, uint32_t first, uint64_t out_off) { return ga + first == out_off; }

/* LDS of k_take: k_batch's tables, payload rows and wave records, then the
 * round's record (HBT_MISC_BYTES), the marks (NL) and a stream's first byte
 * in the round by ordinal (NL + 2), then the staging -- which between two
 * rounds' copy-out and emission is free and holds the streams' data_off and
 * bits by ordinal (NL + 1 each): they are read before the payload is loaded. */
#define HBT_MISC_BYTES 160u
HH_FD uint32_t hbt_extra_bytes(uint32_t W) {
    const uint32_t NL = HB_NR * W;
    return ((NL + (NL + 2u)) * 4u + HBT_MISC_BYTES + 15u) & ~15u;
}
HH_FD uint32_t hbt_union_bytes(uint32_t S, uint32_t minlen, uint32_t W) {
    const uint32_t st = hb_stage_bytes(S, minlen, W), sd = (2u * (HB_NR * W + 1u) * 8u + 15u) & ~15u;
    return st > sd ? st : sd;
}
HH_FD uint32_t hbt_lds_bytes(uint32_t tabb, uint32_t S, uint32_t minlen, uint32_t W) {
    return ((tabb + hb_pay_bytes(S, W) + hb_misc_bytes() + 15u) & ~15u) + hbt_extra_bytes(W) + hbt_union_bytes(S, minlen, W);
}
HH_FD uint32_t hbt_pick_waves(uint32_t tabb, uint32_t S, uint32_t minlen, uint32_t lds) {
    uint32_t W = HB_WMAX;
    while (W && hbt_lds_bytes(tabb, S, minlen, W) > lds) W--;
    return W;
}

#endif
