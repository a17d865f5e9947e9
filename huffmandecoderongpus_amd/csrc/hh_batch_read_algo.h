/*
 * hh_batch_read_algo.h -- the rules of a range read over a block-coded
 * buffer (hh_decode_blocks_read; hh_batch_read.hip: k_read_count,
 * k_read_scan, k_read_fill), __host__ __device__: the kernels run them per
 * read and per piece, the test-only emulator (tests/emu/
 * hh_blocks_read_emu.cpp) runs the same functions on the host.
 *
 * The buffer holds n_syms symbols in blocks of B = block_syms, block b the
 * symbols [b B, min(n_syms, (b + 1) B)), each a stream of its own from the
 * root.  A read (src_off, len, dst_off) wants the symbols [src_off, src_off
 * + len) at dst_off of the output:
 *
 *   valid   hbr_read_ok: src_off + len <= n_syms and dst_off + len <=
 *           out_bytes, neither sum formed.  An invalid read gets no piece.
 *   pieces  hbr_blocks: one per block the read touches, none for len = 0.
 *           Piece j of a read is its part in block src_off / B + j
 *           (hbr_piece): the window [skip, skip + cap) of that block's
 *           symbols, delivered at out_off.
 *   budget  hbr_budget: P = out_bytes / B + 2 m slots.  A read of len bytes
 *           touches at most (len - 1) / B + 2 <= len / B + 2 blocks, and
 *           reads with disjoint destinations have lengths that add up to at
 *           most out_bytes, so their pieces never exceed P.  The host sizes
 *           workspace and grids by P alone; a read whose pieces would end
 *           beyond P (hbr_fits; overlapping destinations only) gets none.
 */
#ifndef HH_BATCH_READ_ALGO_H_
#define HH_BATCH_READ_ALGO_H_

#include <stdint.h>

#include "hh_fsm_algo.h"
#include "hiphuff.h"

/* 1: the read lies inside the data and its destination inside the output. */
HH_FD int hbr_read_ok(uint64_t src_off, uint64_t len, uint64_t dst_off, uint64_t n_syms, uint64_t out_bytes) {
    if (src_off > n_syms || len > n_syms - src_off) return 0;
    if (dst_off > out_bytes || len > out_bytes - dst_off) return 0;
    return 1;
}

/* The blocks a valid read touches (B > 0; src_off + len <= n_syms: no overflow). */
HH_FD uint64_t hbr_blocks(uint64_t src_off, uint64_t len, uint64_t B) {
    if (len == 0) return 0;
    return (src_off + len - 1u) / B - src_off / B + 1u;
}

/* Piece j < hbr_blocks of a valid read: its block, the window of the block's
 * symbols and where they go. */
HH_FD void hbr_piece(uint64_t src_off, uint64_t len, uint64_t dst_off, uint64_t B, uint64_t j, uint64_t *blk,
                     uint64_t *skip, uint64_t *cap, uint64_t *out_off) {
    const uint64_t b = src_off / B + j, b0 = b * B;           /* (b0 < src_off + len <= n_syms) */
    const uint64_t lo = src_off > b0 ? src_off : b0;
    const uint64_t end = src_off + len, hi = end - b0 < B ? end : b0 + B;   /* (b0 + B may pass 2^64: not formed then) */
    *blk = b;
    *skip = lo - b0;
    *cap = hi - lo;
    *out_off = dst_off + (lo - src_off);
}

/* The piece budget of m reads into out_bytes of output; 0: 2^32 - 1 slots or
 * more (unsupported), *P untouched. */
HH_FD int hbr_budget(uint64_t out_bytes, uint64_t B, uint64_t m, uint64_t *P) {
    const uint64_t lim = 0xffffffffull;
    if (B == 0 || m > lim / 2u) return 0;
    const uint64_t q = out_bytes / B;
    if (q >= lim || q + 2u * m >= lim) return 0;
    *P = q + 2u * m;
    return 1;
}

/* a + b, saturating (piece counts of reads that do not fit anyway) */
HH_FD uint64_t hbr_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

/* 1: a read of cnt pieces whose first slot is start ends inside the budget. */
HH_FD int hbr_fits(uint64_t start, uint64_t cnt, uint64_t P) { return cnt == 0 || (start <= P && cnt <= P - start); }

/* The read that owns slot s < total: the last one whose first slot is at or
 * below s (reads without pieces share their successor's first slot and come
 * before it; reads that did not fit start at or beyond the total). */
HH_FD uint64_t hbr_owner(const uint64_t *start, uint64_t m, uint64_t s) {
    uint64_t lo = 0, hi = m;                                  /* first read with start > s */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (start[mid] <= s) lo = mid + 1u; else hi = mid;
    }
    return lo - 1u;
}

#endif
