// hh_blocks_read_emu.cpp -- TEST-ONLY host run of a range read over a
// block-coded buffer (hh_decode_blocks_read): the plan's rules
// (hh_batch_read_algo.h: k_read_count, k_read_scan, k_read_fill of
// hh_batch_read.hip) read by read and slot by slot, and k_batch's windowed
// rounds (hh_batch_algo.h: hb_window, hb_window_done) lane by lane, as
// hh_batch_emu.cpp runs the plain batch -- with the rounds walked per piece
// reported, so that the early stop is checked without a GPU.  Nothing in the
// product links this file (tests/emu/libhh_emu.so).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hh_algo.h"
#include "hh_batch_algo.h"
#include "hh_batch_plan_algo.h"
#include "hh_batch_read_algo.h"
#include "hh_internal.h"
#include "hiphuff.h"

static hh_tables g_T;
static hh_fsm_tables g_F;

namespace {
struct ByteSink {
    uint8_t *p;
    void put(uint64_t e) {
        for (uint32_t i = 0; i < HH_FSM_ET_NSYM(e); i++) *p++ = (uint8_t)(HH_FSM_ET_SYMS(e) >> (8 * i));
    }
};
}  // namespace

extern "C" {

uint32_t hh_blocks_read_window(uint64_t base, uint32_t n, uint64_t skip, uint64_t cap, uint32_t *from) {
    return hb_window(base, n, skip, cap, from);
}

int32_t hh_blocks_read_ok(uint64_t src_off, uint64_t len, uint64_t dst_off, uint64_t n_syms, uint64_t out_bytes) {
    return hbr_read_ok(src_off, len, dst_off, n_syms, out_bytes);
}

// 0: the budget is 2^32 - 1 or more (or block_syms is 0); *P untouched then.
int32_t hh_blocks_read_budget(uint64_t out_bytes, uint64_t block_syms, uint64_t m, uint64_t *P) {
    return hbr_budget(out_bytes, block_syms, m, P);
}

// The plan of m reads (rows of src_off, len, dst_off) over n_syms symbols in
// blocks of B, into out_bytes of output, with P slots; index: the blocks'
// (data_off, bits, out_off, cap) rows, data_bytes the payload's size.
// rstat[i]: HH_OK or HH_ERR_ARG (no piece); first[i]: the read's first slot;
// *total: the slots that hold a piece; piece: P rows of (owner, block, skip,
// cap, out_off, data_off, bits, key byte), the owner ~0 for padding.  Returns
// HH_OK, or HH_ERR_ARG for B == 0.
int32_t hh_blocks_read_plan_emu(const uint64_t *reads, uint64_t m, uint64_t n_syms, uint64_t B, uint64_t out_bytes,
                                uint64_t P, const uint64_t *index, uint64_t data_bytes, uint64_t round_bits,
                                int32_t *rstat, uint64_t *first, uint64_t *total, uint64_t *piece) {
    if (B == 0 || round_bits == 0) return HH_ERR_ARG;
    std::vector<uint64_t> start(m), copy(3 * m, 0);
    // k_read_count
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t *r = reads + 3 * i;
        const bool ok = hbr_read_ok(r[0], r[1], r[2], n_syms, out_bytes) != 0;
        start[i] = ok ? hbr_blocks(r[0], r[1], B) : 0;
        for (int f = 0; f < 3; f++) copy[3 * i + f] = ok ? r[f] : 0;
        rstat[i] = ok ? HH_OK : HH_ERR_ARG;
    }
    // k_read_scan
    uint64_t carry = 0, tot = ~0ull;
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t c = start[i];
        start[i] = carry;
        if (!hbr_fits(carry, c, P)) {
            rstat[i] = HH_ERR_ARG;
            if (carry < tot) tot = carry;
        }
        carry = hbr_sat_add(carry, c);
    }
    if (carry < tot) tot = carry;
    if (tot > P) tot = P;
    *total = tot;
    for (uint64_t i = 0; i < m; i++) first[i] = start[i];
    // k_read_fill
    for (uint64_t s = 0; s < P; s++) {
        uint64_t *p = piece + 8 * s;
        for (int f = 0; f < 8; f++) p[f] = 0;
        p[0] = ~0ull;
        if (s >= tot) continue;
        const uint64_t i = hbr_owner(start.data(), m, s);
        if (i >= m) return HH_ERR_INTERNAL;
        const uint64_t *r = copy.data() + 3 * i;
        uint64_t blk, skip, cap, out_off;
        hbr_piece(r[0], r[1], r[2], B, s - start[i], &blk, &skip, &cap, &out_off);
        const uint64_t data_off = index[4 * blk], bits = index[4 * blk + 1];
        p[0] = i;
        p[1] = blk;
        p[2] = skip;
        p[3] = cap;
        p[4] = out_off;
        if (hbp_item_ok(data_off, bits, 0, 0, data_bytes, 0)) {
            p[5] = data_off;
            p[6] = bits;
            p[7] = hbp_bin(bits, round_bits);
        } else {
            p[7] = HBP_INVALID;
        }
    }
    return HH_OK;
}

// k_batch's rounds for window pieces: n rows of (data_off, bits, out_off,
// cap, skip), decoded with W tiles per round into out.  S = 0: the decoder's
// default region bits; K = 0: 6.  len[i]: the bytes delivered; status[i];
// rounds[i]: the rounds walked; *rb the bits of a round.  Returns HH_OK or an
// argument error.
int64_t hh_blocks_read_emu_decode(const int32_t *izero, const int32_t *ione, const uint8_t *sym, int32_t nodes,
                                  const uint8_t *data, uint64_t data_bytes, const uint64_t *pieces, uint64_t n,
                                  uint32_t S, uint32_t K, uint32_t W, uint8_t *out, uint64_t out_bytes, uint64_t *len,
                                  int32_t *status, uint64_t *rounds, uint64_t *rb) {
    hh_tree tree = {nodes, izero, ione, sym};
    int rc = hh_tables_build(&tree, &g_T);
    if (rc) return rc;
    if (S == 0)
        S = hh_fsm_region_bits(hh_fsm_nstates(&g_T), (uint32_t)g_T.len_gcd, hh_pick_region_bits((uint32_t)g_T.len_gcd));
    if (S < 32 || S % 32 || W < 1 || W > HB_WMAX) return HH_ERR_ARG;
    rc = hh_fsm_build(&g_T, S, K, &g_F);
    if (rc) return rc;
    uint32_t G = hh_fsm_pick_head(&g_T, S, g_F.K);
    if (G > S) G = 0;
    const hb_view F = {g_F.et, g_F.er, g_F.b1, g_F.tsym, g_F.K, g_F.r, S};
    const uint32_t NL = HB_NR * W;
    const uint64_t RB = (uint64_t)NL * S;
    *rb = RB;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *it = pieces + 5 * i;
        if (!hbp_item_ok(it[0], it[1], it[2], it[3], data_bytes, out_bytes)) return HH_ERR_ARG;
    }
    std::vector<uint32_t> ent(NL), x(NL), cnt(NL), nb(NL);
    std::vector<int> whole(NL), at_end(NL);
    std::vector<uint8_t> stg;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t data_off = pieces[5 * i], bits = pieces[5 * i + 1], out_off = pieces[5 * i + 2];
        const uint64_t cap = pieces[5 * i + 3], skip = pieces[5 * i + 4];
        std::vector<uint32_t> wv((bits + 31) / 32 + NL * (S / 32) + 8, 0u);
        memcpy(wv.data(), data + data_off, (size_t)((bits + 31) / 32 * 4 < data_bytes - data_off ? (bits + 31) / 32 * 4
                                                                                                  : data_bytes - data_off));
        const uint32_t *w = wv.data();
        uint64_t base = 0, got = 0, walked = 0;
        uint32_t carry = 0;
        int fail = 0;
        for (uint64_t R0 = 0; cap && R0 < bits; R0 += RB) {
            walked++;
            hb_bits b;
            hb_no_sink none;
            for (uint32_t j = 0; j < NL; j++) {
                const uint64_t R = R0 + (uint64_t)j * S;
                nb[j] = hb_span(R, S, bits, &whole[j], &at_end[j]);
                ent[j] = j ? 0u : carry;
                if (j && G && nb[j]) {
                    hb_bits_init(&b, w, R - G);
                    ent[j] = hb_guess(&F, &b, G);
                }
                hb_bits_init(&b, w, R);
                x[j] = hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], none, &cnt[j]);
            }
            for (uint32_t fr = 0;; fr++) {
                const std::vector<uint32_t> px = x;
                int any = 0;
                for (uint32_t j = 0; j < NL; j++) {
                    if (!hb_fix(j, nb[j], j ? px[j - 1] : carry, &ent[j])) continue;
                    any = 1;
                    hb_bits_init(&b, w, R0 + (uint64_t)j * S);
                    x[j] = hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], none, &cnt[j]);
                }
                if (!any) break;
                if (fr >= HB_FIX_BOUND(W)) { fail = 1; break; }
            }
            uint32_t tot = 0, from = 0;
            for (uint32_t j = 0; j < NL; j++) tot += cnt[j];
            if (tot > W * hb_tile_syms(S, (uint32_t)g_T.minlen)) fail = 1;     // (the kernel's staging)
            const uint32_t keep = hb_window(base, tot, skip, cap, &from);
            // rounds before the window are counted only
            if (!fail && keep) {
                stg.assign(tot + 8, 0);
                uint32_t L = 0;
                for (uint32_t j = 0; j < NL; j++) {
                    ByteSink sink = {stg.data() + L};
                    uint32_t n2 = 0;
                    hb_bits_init(&b, w, R0 + (uint64_t)j * S);
                    hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], sink, &n2);
                    if (n2 != cnt[j]) return HH_ERR_INTERNAL;
                    L += cnt[j];
                }
                // the round's byte t belongs at out_off + base - skip + t
                memcpy(out + (out_off + base - skip + from), stg.data() + from, keep);
                got += keep;
            }
            base += tot;
            carry = x[NL - 1];
            if (hb_window_done(base, skip, cap)) break;
        }
        len[i] = got;
        status[i] = fail ? HH_ERR_INTERNAL : got < cap ? HH_ERR_FORMAT : HH_OK;
        rounds[i] = walked;
    }
    return HH_OK;
}

}  // extern "C"
