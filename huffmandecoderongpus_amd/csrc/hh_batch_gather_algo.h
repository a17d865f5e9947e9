/*
 * hh_batch_gather_algo.h -- the rules of a gathered range read over a
 * block-coded buffer (hh_decode_blocks_gather; hh_batch_gather.hip) that are
 * not already hh_batch_read_algo.h's, __host__ __device__: the kernels run
 * them per block, per piece and per round, the test-only emulator
 * (tests/emu/hh_blocks_gather_emu.cpp) runs the same functions on the host.
 *
 * The reads become pieces exactly as for hh_decode_blocks_read (hbr_*: one
 * piece per read and touched block, in slot order, inside the budget P).
 * Then the pieces are grouped by block and every touched block is walked
 * once, for all its pieces:
 *
 *   blocks  hbg_blocks: nb = ceil(n_syms / B), refused from 2^32 - 1 on (the
 *           call keeps a few words per block, and a block number is a u32).
 *   group   a valid piece adds 1 to its block's count and folds its end
 *           hbg_piece_end = skip + cap into the block's end (a maximum).  The
 *           exclusive scan of the counts (hbg_scan_step, block by block) is a
 *           block's first position in the list of pieces; the blocks with a
 *           count (hbg_touched) are the walks, T of them.  A piece takes
 *           position first + (a rank among its block's pieces, in any
 *           order): nothing below depends on the order inside a block.
 *   walk    rounds as k_batch's (hh_batch_algo.h); a round of n bytes at
 *           base is emitted when one piece at least has bytes in it
 *           (hb_window), once, and every such piece copies its bytes out.
 *           The walk ends after the round with which base + n reaches the
 *           block's end (hbg_walk_done), or with the stream.
 *   result  after the last round, from the symbols `seen` by then: a piece
 *           has hbg_piece_len bytes delivered, HH_ERR_FORMAT when that is
 *           less than its cap (hbg_piece_status).
 *   copy    hbg_copy_split: a piece's bytes of a round go to dst .. dst +
 *           keep as single bytes up to the first 16-byte boundary, whole
 *           16-byte stores, single bytes again: never a byte outside.
 */
#ifndef HH_BATCH_GATHER_ALGO_H_
#define HH_BATCH_GATHER_ALGO_H_

#include <stdint.h>

#include "hh_fsm_algo.h"
#include "hiphuff.h"

#define HBG_SMALL 32u                /* a round's part of a piece up to this many bytes: one lane, byte by byte */

/* The blocks of n_syms symbols in blocks of B; 0: B is 0 or they are 2^32 - 1
 * or more (unsupported), *nb untouched. */
HH_FD int hbg_blocks(uint64_t n_syms, uint64_t B, uint64_t *nb) {
    if (B == 0) return 0;
    const uint64_t q = n_syms / B + (n_syms % B != 0);
    if (q >= 0xffffffffull) return 0;
    *nb = q;
    return 1;
}

/* A piece's end inside its block (skip + cap <= the block's symbols: no overflow). */
HH_FD uint64_t hbg_piece_end(uint64_t skip, uint64_t cap) { return skip + cap; }

/* 1: the block has a valid piece, i.e. it is walked. */
HH_FD uint32_t hbg_touched(uint32_t cnt) { return cnt != 0u; }

/* One step of the exclusive scan over the blocks: block b's first list
 * position and walk ordinal are the sums before it. */
HH_FD void hbg_scan_step(uint32_t cnt, uint32_t *pieces, uint32_t *walks, uint32_t *first, uint32_t *ord) {
    *first = *pieces;
    *ord = *walks;
    *pieces += cnt;
    *walks += hbg_touched(cnt);
}

/* 1: no later round holds a byte of any of the block's pieces (seen = base +
 * the round's bytes, end the largest skip + cap). */
HH_FD int hbg_walk_done(uint64_t seen, uint64_t end) { return seen >= end; }

/* The bytes a piece [skip, skip + cap) got from a walk that saw `seen` symbols. */
HH_FD uint64_t hbg_piece_len(uint64_t seen, uint64_t skip, uint64_t cap) {
    if (seen <= skip) return 0u;
    return seen - skip < cap ? seen - skip : cap;
}

HH_FD int32_t hbg_piece_status(int fail, uint64_t len, uint64_t cap) {
    return fail ? HH_ERR_INTERNAL : len < cap ? HH_ERR_FORMAT : HH_OK;
}

/* keep bytes to the address dst: *head single bytes, then *body stores of 16
 * aligned bytes, then keep - *head - 16 *body single bytes. */
HH_FD void hbg_copy_split(uint64_t dst, uint32_t keep, uint32_t *head, uint32_t *body) {
    const uint32_t h = (uint32_t)((16u - (dst & 15u)) & 15u);
    *head = h < keep ? h : keep;
    *body = (keep - *head) / 16u;
}

#endif
