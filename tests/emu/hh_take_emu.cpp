// hh_take_emu.cpp -- TEST-ONLY host emulation of the record take
// (hh_decode_batch_take; csrc/hh_batch_take.hip).  Runs the plan record by
// record and k_take's packed rounds lane by lane with the rules the kernels
// compile (hh_batch_take_algo.h, hh_batch_algo.h): lengths, offsets and
// fates, the streams' slots, the cut into shares, and per round the marks and
// their maximum scan, the lanes' regions of their own streams, exact entries
// and guesses, fix rounds, the scan, the owners' settling, and the copy-out
// as one range or lane by lane.  A forced share and any W make a geometry of
// several workgroups and short rounds from a few hundred records.  Every
// store is checked against the record's range before it is made.  Nothing in
// the product links this file (tests/emu/libhh_emu.so).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hh_algo.h"
#include "hh_batch_algo.h"
#include "hh_batch_take_algo.h"
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
struct Rec {
    uint64_t data_off, bits, len;
};
}  // namespace

extern "C" {

// The rules alone, for the tests of their corners.
int32_t hh_take_row_ok(uint64_t r, uint64_t nrec, uint64_t data_off, uint64_t bits, uint64_t data_bytes) {
    return hbt_row_ok(r, nrec, data_off, bits, data_bytes);
}
int32_t hh_take_fate(int32_t ok, uint64_t bits, uint64_t len, uint64_t end, uint64_t out_bytes) {
    return hbt_fate(ok, bits, len, end, out_bytes);
}
uint64_t hh_take_sat_add(uint64_t a, uint64_t b) { return hbt_sat_add(a, b); }
uint64_t hh_take_share(uint64_t nslots, uint32_t grid, uint32_t NL, uint64_t forced) {
    return hbt_share(nslots, grid, NL, forced);
}
uint32_t hh_take_pick_waves(uint32_t tabb, uint32_t S, uint32_t minlen, uint32_t lds, uint32_t *batch_w) {
    *batch_w = hb_pick_waves(tabb, S, minlen, lds);
    return hbt_pick_waves(tabb, S, minlen, lds);
}

// index: nrec rows of hh_batch_item's fields; ids: m ids or NULL (m == nrec).
// S = 0: the decoder's default region bits; K = 0: 6.  share != 0: a
// workgroup's slots (rounded up to rounds), as many workgroups as that takes;
// else `grid` workgroups.  summary: total_len, n_failed, first_failed,
// first_status.  stats: [0] S  [1] G  [2] K  [3] rounds  [4] fix rounds that
// changed a lane  [5] the most of them in one round  [6] regions counted
// again  [7] streams  [8] slots  [9] workgroups with a stream  [10] rounds
// copied out as one range  [11] rounds copied out lane by lane  [12] the most
// streams in one round.  Returns HH_OK or what the C call's host checks
// return; HH_ERR_INTERNAL when a rule of the emulation itself breaks.
int64_t hh_take_emu(const int32_t *izero, const int32_t *ione, const uint8_t *sym, int32_t nodes, const uint8_t *data,
                    uint64_t data_bytes, const uint64_t *index, uint64_t nrec, const uint64_t *ids, uint64_t m,
                    uint32_t S, uint32_t K, uint32_t W, uint64_t share, uint32_t grid, uint8_t *out, uint64_t out_bytes,
                    uint64_t *out_offs, int32_t *status, int64_t *summary, int64_t *stats) {
    for (int i = 0; i < 13; i++) stats[i] = 0;
    if (!ids && m != nrec) return HH_ERR_ARG;
    summary[0] = summary[1] = 0;
    summary[2] = 0xffffffffll;
    summary[3] = HH_OK;
    if (m == 0) return HH_OK;
    if (m >= 0xffffffffull || nrec >= 0xffffffffull) return HH_ERR_UNSUPPORTED;
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
    stats[0] = S;
    stats[1] = G;
    stats[2] = g_F.K;
    const hb_view F = {g_F.et, g_F.er, g_F.b1, g_F.tsym, g_F.K, g_F.r, S};
    const uint32_t NL = HB_NR * W, SW = S / 32u, RW = hb_row_words(S);

    // the plan
    std::vector<Rec> rec(m);
    std::vector<hbt_desc> desc;
    uint64_t off = 0, nslots = 0;
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t r = ids ? ids[j] : j;
        int ok = 0;
        rec[j] = Rec{0, 0, 0};
        if (r < nrec) {
            const uint64_t *it = index + 4 * r;
            ok = hbt_row_ok(r, nrec, it[0], it[1], data_bytes);
            if (ok) rec[j] = Rec{it[0], it[1], it[3]};
        }
        out_offs[j] = off;
        const uint64_t end = hbt_sat_add(off, rec[j].len);
        const int32_t f = hbt_fate(ok, rec[j].bits, rec[j].len, end, out_bytes);
        status[j] = f == HBT_STREAM ? HH_ERR_INTERNAL : f;
        if (f == HBT_STREAM) {
            desc.push_back(hbt_desc{rec[j].data_off, rec[j].bits, nslots, off, rec[j].len, j});
            nslots = hbt_sat_add(nslots, hbt_regions(rec[j].bits, S));
        }
        off = end;
    }
    out_offs[m] = off;
    const uint32_t ns = (uint32_t)desc.size();
    stats[7] = ns;
    stats[8] = (int64_t)nslots;
    if (nslots == ~0ull) return HH_ERR_INTERNAL;
    if (share) {
        const uint64_t sh = hbt_share(nslots, 1u, NL, share);
        grid = (uint32_t)(nslots / sh + (nslots % sh != 0));
        if (!grid) grid = 1;
    }
    if (!grid) return HH_ERR_ARG;
    const uint64_t sh = hbt_share(nslots, grid, NL, share);
    std::vector<uint32_t> cut(grid + 1u);
    for (uint32_t e = 0; e < grid; e++) cut[e] = hbt_edge(desc.data(), ns, nslots, sh, e);
    cut[grid] = ns;

    auto word = [&](uint64_t w) -> uint32_t {
        if (w * 4u + 4u > data_bytes) return 0u;
        uint32_t v;
        memcpy(&v, data + w * 4u, 4);
        return v;
    };
    std::vector<uint32_t> pay((size_t)NL * RW + 8u), mk(NL), hd(NL + 2u), ent(NL), x(NL), cnt(NL), nb(NL), mv(NL), Lo(NL);
    std::vector<uint64_t> q(NL), doff(NL), bits(NL);
    std::vector<int> whole(NL), at_end(NL), exact(NL);
    std::vector<uint8_t> stg;
    // a store of `n` bytes for taken record j at output offset o
    auto store_ok = [&](uint64_t j, uint64_t o, uint64_t n) {
        return o >= out_offs[j] && o + n <= out_offs[j + 1] && o + n <= out_bytes;
    };

    for (uint32_t wg = 0; wg < grid; wg++) {
        const uint32_t s0 = cut[wg], s1 = cut[wg + 1];
        if (s0 >= s1) continue;
        stats[9]++;
        const uint64_t base0 = desc[s0].slot0;
        uint32_t nxt = s0, c_has = 0, carry = 0;
        hbt_desc cd = {0, 0, 0, 0, 0, 0};
        uint64_t c_q = 0, c_cnt = 0;
        for (uint64_t lo = 0; c_has || nxt < s1; lo += NL) {
            stats[3]++;
            // the owners: thread t looks at stream nxt + t
            std::fill(mk.begin(), mk.end(), 0u);
            std::vector<uint32_t> spos(NL, 0u);
            std::vector<int> own(NL, 0);
            for (uint32_t t = 0; t < NL && (uint64_t)nxt + t < s1; t++) {
                const uint64_t sl = desc[nxt + t].slot0 - base0;
                if (sl >= lo && sl - lo < NL) {
                    own[t] = 1;
                    spos[t] = (uint32_t)(sl - lo);
                    if (mk[spos[t]]) return HH_ERR_INTERNAL;
                    mk[spos[t]] = hbt_mark(t + 1u, spos[t]);
                }
            }
            const uint64_t ga = c_has ? cd.out_off + c_cnt : desc[nxt].out_off;
            uint32_t run = 0;
            for (uint32_t j = 0; j < NL; j++) mv[j] = run = mk[j] > run ? mk[j] : run;
            const uint32_t o_last = hbt_mark_ord(mv[NL - 1u]);
            if (!o_last && !c_has) return HH_ERR_INTERNAL;
            if ((int64_t)(o_last + c_has) > stats[12]) stats[12] = o_last + c_has;
            for (uint32_t j = 0; j < NL; j++) {
                const uint32_t o = hbt_mark_ord(mv[j]);
                if (!o && !c_has) return HH_ERR_INTERNAL;
                q[j] = hbt_region_of(j, mv[j], c_q);
                doff[j] = o ? desc[nxt + o - 1u].data_off : cd.data_off;
                bits[j] = o ? desc[nxt + o - 1u].bits : cd.bits;
                nb[j] = hb_span(q[j] * S, S, bits[j], &whole[j], &at_end[j]);
                uint32_t *row = pay.data() + (size_t)j * RW;
                if (nb[j])
                    for (uint32_t k = 0; k < SW; k++) row[k] = word(doff[j] / 4u + q[j] * SW + k);
            }
            hb_bits b;
            hb_no_sink none;
            for (uint32_t j = 0; j < NL; j++) {
                exact[j] = hbt_exact(j, q[j]);
                ent[j] = exact[j] ? hbt_entry(q[j], carry) : 0u;
                if (!exact[j] && G && nb[j]) {
                    hb_bits_init(&b, pay.data() + (size_t)(j - 1u) * RW, S - G);
                    ent[j] = hb_guess(&F, &b, G);
                }
                hb_bits_init(&b, pay.data() + (size_t)j * RW, 0);
                x[j] = hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], none, &cnt[j]);
            }
            uint32_t fr = 0;
            for (;; fr++) {
                const std::vector<uint32_t> px = x;
                int any = 0;
                for (uint32_t j = 0; j < NL; j++) {
                    if (!hbt_fix(exact[j], nb[j], j ? px[j - 1] : carry, &ent[j])) continue;
                    any = 1;
                    stats[6]++;
                    hb_bits_init(&b, pay.data() + (size_t)j * RW, 0);
                    x[j] = hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], none, &cnt[j]);
                }
                if (!any) break;
                if (fr >= HB_FIX_BOUND(W)) return HH_ERR_INTERNAL;
            }
            stats[4] += fr;
            if ((int64_t)fr > stats[5]) stats[5] = fr;
            // the scan, the streams' first bytes, the emission
            uint32_t tot = 0;
            for (uint32_t j = 0; j < NL; j++) {
                Lo[j] = tot;
                if (j == 0 || q[j] == 0) hd[hbt_mark_ord(mv[j])] = tot;
                tot += cnt[j];
            }
            hd[o_last + 1u] = tot;
            if (tot > W * hb_tile_syms(S, (uint32_t)g_T.minlen)) return HH_ERR_INTERNAL;   // (the kernel's staging)
            stg.assign(tot + 8u, 0);
            for (uint32_t j = 0; j < NL; j++) {
                ByteSink sink = {stg.data() + Lo[j]};
                uint32_t n2 = 0;
                hb_bits_init(&b, pay.data() + (size_t)j * RW, 0);
                hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], sink, &n2);
                if (n2 != cnt[j]) return HH_ERR_INTERNAL;
            }
            // the owners settle their streams
            int bad = 0;
            uint32_t n_has = 0;
            hbt_desc nd = cd;
            uint64_t n_q = 0, n_cnt = 0;
            for (uint32_t t = 0; t < NL; t++) {
                if (!own[t]) continue;
                const hbt_desc &od = desc[nxt + t];
                const uint32_t first = hd[t + 1u], nr = hd[t + 2u] - first;
                const int ended = spos[t] + hbt_regions(od.bits, S) <= NL;
                int32_t st;
                if (hbt_settle(0u, nr, od.len, ended, &st) || !hbt_in_place(ga, first, od.out_off)) bad = 1;
                if (ended) {
                    status[od.j] = st;
                } else {
                    if (n_has) return HH_ERR_INTERNAL;
                    n_has = 1; nd = od; n_q = NL - spos[t]; n_cnt = nr;
                }
            }
            if (c_has) {
                const uint32_t nr = hd[1] - hd[0];
                const int ended = hbt_regions(cd.bits, S) - c_q <= NL;
                int32_t st;
                if (hbt_settle(c_cnt, nr, cd.len, ended, &st)) bad = 1;
                if (ended) {
                    status[cd.j] = st;
                } else {
                    if (n_has) return HH_ERR_INTERNAL;
                    n_has = 1; n_q = c_q + NL; n_cnt = c_cnt + nr;
                }
            }
            if (!bad) {
                stats[10]++;
                // one range: every byte of it must be a byte of the record whose lane holds it
                for (uint32_t j = 0; j < NL; j++) {
                    const uint32_t o = hbt_mark_ord(mv[j]);
                    if (cnt[j] && !store_ok(o ? desc[nxt + o - 1u].j : cd.j, ga + Lo[j], cnt[j])) return HH_ERR_INTERNAL;
                }
                memcpy(out + ga, stg.data(), tot);
            } else {
                stats[11]++;
                for (uint32_t j = 0; j < NL; j++) {
                    if (!cnt[j]) continue;
                    const uint32_t o = hbt_mark_ord(mv[j]);
                    const hbt_desc &sd = o ? desc[nxt + o - 1u] : cd;
                    const uint64_t pos = (o ? 0u : c_cnt) + (Lo[j] - hd[o]);
                    const uint32_t keep = hb_clip(pos, cnt[j], sd.len);
                    if (keep && !store_ok(sd.j, sd.out_off + pos, keep)) return HH_ERR_INTERNAL;
                    memcpy(out + sd.out_off + pos, stg.data() + Lo[j], keep);
                }
            }
            c_has = n_has;
            cd = nd;
            c_q = n_q;
            c_cnt = n_cnt;
            nxt += o_last;
            carry = x[NL - 1u];
        }
    }
    // the summary
    for (uint64_t j = 0; j < m; j++) {
        if (status[j] == HH_OK) {
            summary[0] += (int64_t)(out_offs[j + 1] - out_offs[j]);
        } else {
            if (summary[1]++ == 0) {
                summary[2] = (int64_t)j;
                summary[3] = status[j];
            }
        }
    }
    return HH_OK;
}

}  // extern "C"
