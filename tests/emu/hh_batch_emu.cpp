// hh_batch_emu.cpp -- TEST-ONLY host emulation of the batched decode
// (hh_batch.hip: k_batch).  Runs a workgroup's rounds lane by lane with the
// same tables (hh_fsm_build) and the same rules (hh_batch_algo.h): guesses
// from G-bit heads, counts over the emission tables, fix rounds until no
// lane's entry differs from its predecessor's exit, the scan, emission, and
// the copy-out clipped to each stream's capacity -- for a list of items and
// any number W of tiles per round, so that the decomposition is checked
// against the oracle without a GPU.  Every region's emitted symbols are
// checked against its count.  Nothing in the product links this file
// (tests/emu/libhh_emu.so).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hh_algo.h"
#include "hh_batch_algo.h"
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

// items: n rows of (data_off, bits, out_off, cap), hh_batch_item's fields.
// S = 0: the decoder's default region bits; K = 0: 6.  stats[0] S  [1] G
// [2] K  [3] rounds  [4] fix rounds that changed a lane  [5] the most of them
// in one round  [6] regions counted again.  Returns HH_OK or the status of
// the lowest-index failing stream; argument errors as the C ABI's.
int64_t hh_batch_emu_decode(const int32_t *izero, const int32_t *ione, const uint8_t *sym, int32_t nodes,
                            const uint8_t *data, uint64_t data_bytes, const uint64_t *items, uint64_t n,
                            uint32_t S, uint32_t K, uint32_t W, uint8_t *out, uint64_t out_bytes,
                            uint64_t *out_len, int32_t *status, int64_t *stats) {
    hh_tree tree = {nodes, izero, ione, sym};
    int rc = hh_tables_build(&tree, &g_T);
    if (rc) return rc;
    for (int i = 0; i < 7; i++) stats[i] = 0;
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
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *it = items + 4 * i;
        if (it[0] % 4) return HH_ERR_ARG;
        if (it[1] && (it[0] > data_bytes || (it[1] + 7) / 8 + HH_PAYLOAD_PAD > data_bytes - it[0])) return HH_ERR_ARG;
        if (it[2] > out_bytes || it[3] > out_bytes - it[2]) return HH_ERR_ARG;
    }
    const hb_view F = {g_F.et, g_F.er, g_F.b1, g_F.tsym, g_F.K, g_F.r, S};
    const uint32_t NL = HB_NR * W;
    const uint64_t RB = (uint64_t)NL * S;
    std::vector<uint32_t> ent(NL), x(NL), cnt(NL), nb(NL);
    std::vector<int> whole(NL), at_end(NL);
    std::vector<uint8_t> stg;
    int64_t first = HH_OK;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t data_off = items[4 * i], bits = items[4 * i + 1], out_off = items[4 * i + 2], cap = items[4 * i + 3];
        // the stream's words; what lies past them reads as 0 (the kernel's buffer loads)
        std::vector<uint32_t> wv((bits + 31) / 32 + NL * (S / 32) + 8, 0u);
        memcpy(wv.data(), data + data_off, (size_t)((bits + 31) / 32 * 4 < data_bytes - data_off ? (bits + 31) / 32 * 4
                                                                                                  : data_bytes - data_off));
        const uint32_t *w = wv.data();
        uint64_t base = 0;
        uint32_t carry = 0;
        int fail = 0;
        for (uint64_t R0 = 0; R0 < bits; R0 += RB) {
            stats[3]++;
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
            // fix rounds: every lane looks at its predecessor's exit of the round before
            uint32_t fr = 0;
            for (;; fr++) {
                const std::vector<uint32_t> px = x;
                int any = 0;
                for (uint32_t j = 0; j < NL; j++) {
                    if (!hb_fix(j, nb[j], j ? px[j - 1] : carry, &ent[j])) continue;
                    any = 1;
                    stats[6]++;
                    hb_bits_init(&b, w, R0 + (uint64_t)j * S);
                    x[j] = hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], none, &cnt[j]);
                }
                if (!any) break;
                if (fr >= HB_FIX_BOUND(W)) { fail = 1; break; }
            }
            stats[4] += fr;
            if ((int64_t)fr > stats[5]) stats[5] = fr;
            // scan, emission, the copy-out below the capacity
            uint32_t tot = 0;
            for (uint32_t j = 0; j < NL; j++) tot += cnt[j];
            if (tot > W * hb_tile_syms(S, (uint32_t)g_T.minlen)) fail = 1;     // (the kernel's staging)
            stg.assign(tot + 8, 0);
            uint32_t L = 0;
            for (uint32_t j = 0; j < NL && !fail; j++) {
                ByteSink sink = {stg.data() + L};
                uint32_t n2 = 0;
                hb_bits_init(&b, w, R0 + (uint64_t)j * S);
                hb_region(&F, &b, nb[j], whole[j], at_end[j], ent[j], sink, &n2);
                if (n2 != cnt[j] || (uint32_t)(sink.p - stg.data()) != L + cnt[j]) {
                    fprintf(stderr, "batch emu: stream %llu region %u emitted %u, counted %u\n", (unsigned long long)i, j,
                            n2, cnt[j]);
                    return HH_ERR_INTERNAL;
                }
                L += cnt[j];
            }
            if (!fail) memcpy(out + out_off + base, stg.data(), hb_clip(base, tot, cap));
            base += tot;
            carry = x[NL - 1];
        }
        out_len[i] = base;
        const int32_t s = fail ? HH_ERR_INTERNAL : base > cap ? HH_ERR_CAPACITY : HH_OK;
        if (status) status[i] = s;
        if (s != HH_OK && first == HH_OK) first = s;
    }
    return first;
}

}  // extern "C"
