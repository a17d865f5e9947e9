// hh_blocks_gather_emu.cpp -- TEST-ONLY host run of a gathered range read
// over a block-coded buffer (hh_decode_blocks_gather): the plan up to the
// pieces by hh_batch_read_algo.h's rules, the grouping by block, the walk's
// end, a piece's result and the copy's split by hh_batch_gather_algo.h's --
// the very functions hh_batch_gather.hip's kernels run -- and k_gather's
// merged walk over one block's piece list lane by lane from the hb_*
// functions of hh_batch_algo.h, with the rounds walked and emitted reported.
// Nothing in the product links this file (tests/emu/libhh_emu.so).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hh_algo.h"
#include "hh_batch_algo.h"
#include "hh_batch_gather_algo.h"
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

// 0: block_syms is 0 or the blocks are 2^32 - 1 or more; *nb untouched then.
int32_t hh_blocks_gather_blocks(uint64_t n_syms, uint64_t block_syms, uint64_t *nb) {
    return hbg_blocks(n_syms, block_syms, nb);
}

void hh_blocks_gather_copy_split(uint64_t dst, uint32_t keep, uint32_t *head, uint32_t *body) {
    hbg_copy_split(dst, keep, head, body);
}

// The plan of m reads (rows of src_off, len, dst_off) as
// hh_blocks_read_plan_emu's, then grouped: rstat[i], *total as there; per
// block cnt[b], end[b], bfirst[b]; *T the touched blocks; list: *total rows
// at most (P allocated) of (owner, block, skip, cap, out_off) by list
// position -- block b's at bfirst[b] .. + cnt[b]; key[s]: slot s's key byte
// (HBP_INVALID for a bad index entry).  reverse != 0: the slots are placed
// last first (the order inside a block's list is any).  Returns HH_OK, or
// HH_ERR_ARG / HH_ERR_UNSUPPORTED as the host checks would.
int32_t hh_blocks_gather_plan_emu(const uint64_t *reads, uint64_t m, uint64_t n_syms, uint64_t B, uint64_t out_bytes,
                                  uint64_t P, const uint64_t *index, uint64_t data_bytes, int32_t reverse,
                                  int32_t *rstat, uint64_t *total, uint32_t *cnt, uint64_t *end, uint32_t *bfirst,
                                  uint32_t *T, uint64_t *list, uint8_t *key) {
    if (B == 0) return HH_ERR_ARG;
    uint64_t nb = 0;
    if (!hbg_blocks(n_syms, B, &nb)) return HH_ERR_UNSUPPORTED;
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
    // k_gather_fill
    struct Piece { uint64_t own, blk, skip, cap, out_off; int ok; };
    std::vector<Piece> pc(tot);
    for (uint64_t b = 0; b < nb; b++) { cnt[b] = 0; end[b] = 0; }
    for (uint64_t s = 0; s < tot; s++) {
        const uint64_t i = hbr_owner(start.data(), m, s);
        if (i >= m) return HH_ERR_INTERNAL;
        const uint64_t *r = copy.data() + 3 * i;
        Piece &p = pc[s];
        p.own = i;
        hbr_piece(r[0], r[1], r[2], B, s - start[i], &p.blk, &p.skip, &p.cap, &p.out_off);
        if (p.blk >= nb) return HH_ERR_INTERNAL;
        p.ok = hbp_item_ok(index[4 * p.blk], index[4 * p.blk + 1], 0, 0, data_bytes, 0);
        key[s] = (uint8_t)(p.ok ? 0u : HBP_INVALID);
        if (p.ok) {
            cnt[p.blk]++;
            const uint64_t e = hbg_piece_end(p.skip, p.cap);
            if (e > end[p.blk]) end[p.blk] = e;
        }
    }
    // the scan over the blocks
    uint32_t pieces = 0, walks = 0, ord;
    for (uint64_t b = 0; b < nb; b++) hbg_scan_step(cnt[b], &pieces, &walks, &bfirst[b], &ord);
    *T = walks;
    // k_gather_place
    std::vector<uint32_t> cur(nb, 0);
    for (uint64_t k = 0; k < tot; k++) {
        const uint64_t s = reverse ? tot - 1 - k : k;
        const Piece &p = pc[s];
        if (!p.ok) continue;
        const uint64_t at = bfirst[p.blk] + cur[p.blk]++;
        if (at >= P) return HH_ERR_INTERNAL;
        uint64_t *row = list + 5 * at;
        row[0] = p.own; row[1] = p.blk; row[2] = p.skip; row[3] = p.cap; row[4] = p.out_off;
    }
    return HH_OK;
}

// k_gather's walk of one block (data_off, bits) for its n pieces, rows of
// (out_off, cap, skip), with W tiles per round into out.  S = 0: the
// decoder's default region bits; K = 0: 6.  len[i], status[i]: a piece's
// result; *rounds the rounds walked, *emitted those of them that were
// emitted, *rb the bits of a round.  Returns HH_OK or an argument error.
int64_t hh_blocks_gather_emu_walk(const int32_t *izero, const int32_t *ione, const uint8_t *sym, int32_t nodes,
                                  const uint8_t *data, uint64_t data_bytes, uint64_t data_off, uint64_t bits,
                                  const uint64_t *pieces, uint64_t n, uint32_t S, uint32_t K, uint32_t W, uint8_t *out,
                                  uint64_t out_bytes, uint64_t *len, int32_t *status, uint64_t *rounds,
                                  uint64_t *emitted, uint64_t *rb) {
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
    if (!hbp_item_ok(data_off, bits, 0, 0, data_bytes, 0)) return HH_ERR_ARG;
    uint64_t end = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *p = pieces + 3 * i;
        if (!hbp_item_ok(0, 0, p[0], p[1], 0, out_bytes)) return HH_ERR_ARG;
        if (p[1] && hbg_piece_end(p[2], p[1]) > end) end = hbg_piece_end(p[2], p[1]);
    }
    std::vector<uint32_t> ent(NL), x(NL), cnt(NL), nb(NL);
    std::vector<int> whole(NL), at_end(NL);
    std::vector<uint8_t> stg;
    std::vector<uint32_t> wv((bits + 31) / 32 + NL * (S / 32) + 8, 0u);
    memcpy(wv.data(), data + data_off, (size_t)((bits + 31) / 32 * 4 < data_bytes - data_off ? (bits + 31) / 32 * 4
                                                                                              : data_bytes - data_off));
    const uint32_t *w = wv.data();
    uint64_t base = 0, walked = 0, emit = 0;
    uint32_t carry = 0;
    int fail = 0;
    for (uint64_t R0 = 0; end && R0 < bits; R0 += RB) {      // (a block without a byte wanted is not walked)
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
        int hit = 0;
        for (uint64_t i = 0; !fail && i < n; i++) hit |= hb_window(base, tot, pieces[3 * i + 2], pieces[3 * i + 1], &from) != 0;
        if (hit) {
            emit++;
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
            for (uint64_t i = 0; i < n; i++) {
                const uint64_t out_off = pieces[3 * i], cap = pieces[3 * i + 1], skip = pieces[3 * i + 2];
                const uint32_t keep = hb_window(base, tot, skip, cap, &from);
                if (!keep) continue;
                // head bytes, whole 16-byte blocks, tail bytes (the offsets are the addresses here)
                const uint64_t dst = out_off + (base + from - skip);
                uint32_t head, body;
                hbg_copy_split(dst, keep, &head, &body);
                if (head > keep || head + 16u * body > keep || keep - head - 16u * body >= 16u ||
                    (body && (dst + head) % 16u))
                    return HH_ERR_INTERNAL;
                memcpy(out + dst, stg.data() + from, head);
                for (uint32_t q = 0; q < body; q++) memcpy(out + dst + head + 16u * q, stg.data() + from + head + 16u * q, 16);
                memcpy(out + dst + head + 16u * body, stg.data() + from + head + 16u * body, keep - head - 16u * body);
            }
        }
        base += tot;
        carry = x[NL - 1];
        if (hbg_walk_done(base, end)) break;
    }
    for (uint64_t i = 0; i < n; i++) {
        len[i] = hbg_piece_len(base, pieces[3 * i + 2], pieces[3 * i + 1]);
        status[i] = hbg_piece_status(fail, len[i], pieces[3 * i + 1]);
    }
    *rounds = walked;
    *emitted = emit;
    return HH_OK;
}

}  // extern "C"
