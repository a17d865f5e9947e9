// hh_encr_emu.cpp -- TEST-ONLY host run of the ragged blocked encode
// (hh_encoder_encode_ragged, csrc/hh_encr.hip): its launches one after the
// other, chunk by chunk and tile by tile, with hh_encr_algo.h's rules -- the
// cut, the length pass with loc, the two tiled scans, the items, and the pack
// into a per-chunk image that goes out with plain stores inside and ORs on
// its first and last word.  reverse != 0 packs the chunks last first: a word
// that two chunks share and one of them stores plainly then shows.
// Nothing in the product links this file (tests/emu/libhh_emu.so).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hh_encr_algo.h"
#include "hh_internal.h"
#include "hiphuff.h"

namespace {
const uint32_t TB = 256, PT = 16;       // k_encr_len's and k_encr_pack's threads, symbols per thread

// k_encr_top: nt sums into exclusive ones, HER_TILE a step with the carry.
uint64_t top(std::vector<uint64_t> &sums, uint64_t nt, uint64_t *steps) {
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < nt; t0 += HER_TILE) {
        uint64_t tot = 0;
        for (uint64_t t = t0; t < nt && t < t0 + HER_TILE; t++) {
            const uint64_t v = sums[t];
            sums[t] = carry + tot;
            tot += v;
        }
        carry += tot;
        ++*steps;
    }
    return carry;
}
}  // namespace

extern "C" {

uint64_t hh_encr_record_of(const uint64_t *offs, uint64_t nrec, uint64_t i) { return her_record_of(offs, nrec, i); }
uint64_t hh_encr_lower(const uint64_t *offs, uint64_t nrec, uint64_t t) { return her_lower(offs, nrec, t); }
uint32_t hh_encr_img_alloc(uint32_t maxlen, uint64_t nrec) { return her_img_alloc(maxlen, nrec); }

// The device call's statuses.  out: cap bytes, written below *total_bytes
// only; items: nrec rows of (data_off, bits, out_off, cap), or NULL.  info:
// [0] the largest image in words, [1] the steps of the record scan's top,
// [2] the flag word.
int32_t hh_encr_emu(const int32_t *izero, const int32_t *ione, const uint8_t *sym, int32_t nodes, const uint8_t *syms,
                    uint64_t n, const uint64_t *offs, uint64_t nrec, uint8_t *out, uint64_t cap, uint64_t *items,
                    uint64_t *total_bytes, int32_t reverse, uint64_t *info) {
    *total_bytes = 0;
    info[0] = info[1] = info[2] = 0;
    const hh_tree tree = {nodes, izero, ione, sym};
    uint64_t code[256];
    uint8_t len8[256];
    int rc = hh_codebook(&tree, code, len8);
    if (rc) return rc;
    uint32_t maxlen = 0;
    for (int i = 0; i < 256; i++) maxlen = len8[i] > maxlen ? len8[i] : maxlen;
    if (nrec >= 0xffffffffull) return HH_ERR_UNSUPPORTED;
    const uint64_t nch = n / HER_CH + (n % HER_CH != 0);
    if (nrec == 0) return n == 0 ? HH_OK : HH_ERR_ARG;
    const uint64_t ntc = nch / HER_TILE + 1, ntr = (nrec + HER_TILE - 1) / HER_TILE;
    uint32_t flags = 0;
    std::vector<uint32_t> rlo(nch + 1), loc(nrec, 0xdeadbeefu);
    std::vector<uint64_t> CS(nch + 1, 0), ctile(ntc, 0), start(nrec), bits(nrec), wb(nrec), rtile(ntr, 0);
    // k_encr_cut
    for (uint64_t c = 0; c <= nch; c++) rlo[c] = (uint32_t)her_lower(offs, nrec, c * HER_CH < n ? c * HER_CH : n);
    // k_encr_len
    std::vector<uint32_t> pre(HER_CH);
    for (uint64_t c = 0; c < nch; c++) {
        const uint64_t c0 = c * HER_CH, c1 = n - c0 < HER_CH ? n : c0 + HER_CH;
        uint32_t p = 0;
        for (uint64_t i = c0; i < c0 + HER_CH; i++) {
            pre[i - c0] = p;
            if (i < c1) {
                p += len8[syms[i]];
                if (!len8[syms[i]]) flags |= HER_F_ABSENT;
            }
        }
        CS[c] = p;
        for (uint64_t r = rlo[c]; r < rlo[c + 1]; r++) {
            const uint64_t o = offs[r] - c0;
            if (o < c1 - c0) loc[r] = pre[o];
            else flags |= HER_F_OFFS;
        }
    }
    // k_encr_csums, k_encr_cfirst (every tile adds up the tiles before it)
    for (uint64_t c = 0; c < nch; c++) ctile[c / HER_TILE] += CS[c];
    uint64_t total = 0;
    for (uint64_t t = 0; t < ntc; t++) {
        uint64_t base = 0, x = 0;
        for (uint64_t u = 0; u < t; u++) base += ctile[u];
        for (uint64_t c = t * HER_TILE; c <= nch && c < (t + 1) * HER_TILE; c++) {
            const uint64_t v = c < nch ? CS[c] : 0;
            CS[c] = base + x;
            if (c == nch) total = base + x;
            x += v;
        }
    }
    // k_encr_rsums
    for (uint64_t t = 0; t < ntr; t++)
        for (uint64_t r = t * HER_TILE; r < nrec && r < (t + 1) * HER_TILE; r++) {
            const uint64_t a = offs[r], b = offs[r + 1];
            const bool ok = her_pair_ok(a, b, n) && (r != 0 || a == 0) && (r + 1 != nrec || b == n);
            uint64_t s0 = 0, s1 = 0;
            if (ok) {
                s0 = her_start(CS.data(), a, a == n ? 0u : loc[r], n, total);
                s1 = her_start(CS.data(), b, b == n ? 0u : loc[r + 1], n, total);
            } else {
                flags |= HER_F_OFFS;
            }
            start[r] = s0;
            bits[r] = s1 - s0;
            rtile[t] += her_words(s1 - s0);
        }
    // k_encr_top, k_encr_rfirst
    uint64_t steps = 0;
    const uint64_t words = top(rtile, ntr, &steps);
    info[1] = steps;
    for (uint64_t t = 0; t < ntr; t++) {
        uint64_t x = 0;
        for (uint64_t r = t * HER_TILE; r < nrec && r < (t + 1) * HER_TILE; r++) {
            wb[r] = rtile[t] + x;
            x += her_words(bits[r]);
        }
    }
    // k_encr_items
    if (items && !flags)
        for (uint64_t r = 0; r < nrec; r++) {
            items[4 * r] = 4 * wb[r];
            items[4 * r + 1] = bits[r];
            items[4 * r + 2] = offs[r];
            items[4 * r + 3] = offs[r + 1] - offs[r];
        }
    // the host
    info[2] = flags;
    if (flags) return HH_ERR_ARG;
    if (words * 32 < total) return HH_ERR_INTERNAL;
    *total_bytes = words * 4;
    if (words * 4 > cap) return HH_ERR_CAPACITY;
    memset(out, 0, words * 4);
    // k_encr_pack
    const uint32_t img_alloc = her_img_alloc(maxlen, nrec) > HER_CH ? her_img_alloc(maxlen, nrec) : HER_CH;
    std::vector<uint32_t> mark(HER_CH), img;
    for (uint64_t cc = 0; cc < nch; cc++) {
        const uint64_t c = reverse ? nch - 1 - cc : cc;
        const uint64_t c0 = c * HER_CH, c1 = n - c0 < HER_CH ? n : c0 + HER_CH;
        const uint32_t r0 = rlo[c], r1 = rlo[c + 1];
        std::fill(mark.begin(), mark.end(), 0u);
        for (uint64_t r = r0; r < r1; r++) {
            const uint64_t o = offs[r] - c0;
            if (o < c1 - c0 && mark[o] < (uint32_t)r + 1u) mark[o] = (uint32_t)r + 1u;
        }
        if (r1 == 0 || (mark[0] == 0 && r0 == 0)) { flags |= HER_F_INTERNAL; continue; }
        const uint32_t rf = mark[0] ? mark[0] - 1u : r0 - 1u, rl = r1 - 1u;
        const uint64_t g0 = her_pos(wb[rf], start[rf], CS[c]), gend = her_pos(wb[rl], start[rl], CS[c + 1]);
        const uint64_t W0 = g0 >> 5, nw = gend > g0 ? her_img_words(g0, gend) : 0;
        if (nw == 0 || nw > img_alloc || W0 + nw > words) { flags |= HER_F_INTERNAL; continue; }
        if (nw > info[0]) info[0] = nw;
        img.assign(nw + 2, 0u);
        uint64_t P = CS[c];
        uint32_t em = 0;                                  // (the mark in force: the threads' running maximum)
        for (uint32_t tid = 0; tid < TB; tid++) {
            uint32_t cur = em ? em - 1u : r0 - 1u;
            for (uint32_t k = 0; k < PT; k++) {
                const uint64_t i = c0 + (uint64_t)tid * PT + k;
                const uint32_t m = mark[tid * PT + k];
                em = m > em ? m : em;
                if (i >= c1) continue;
                if (m) cur = m - 1u;
                if (cur != her_record_of(offs, nrec, i)) flags |= HER_F_INTERNAL;   // (the marks against the rule)
                const uint32_t l = len8[syms[i]];
                const uint64_t cd = code[syms[i]];
                const uint64_t g = her_pos(wb[cur], start[cur], P) - 32 * W0;
                P += l;
                if (g + l > 32 * nw) { flags |= HER_F_INTERNAL; continue; }
                const uint32_t w = (uint32_t)g >> 5, o = (uint32_t)g & 31u;
                const uint64_t v = cd << o;
                if (l) img[w] |= (uint32_t)v;
                if (o + l > 32u) img[w + 1] |= (uint32_t)(v >> 32);
                if (o + l > 64u) img[w + 2] |= (uint32_t)(cd >> (64u - o));
            }
        }
        for (uint64_t i = 0; i < nw; i++) {
            uint32_t word;
            memcpy(&word, out + 4 * (W0 + i), 4);
            word = (i == 0 || i + 1 == nw) ? (word | img[i]) : img[i];
            memcpy(out + 4 * (W0 + i), &word, 4);
        }
    }
    info[2] = flags;
    return flags ? HH_ERR_INTERNAL : HH_OK;
}

}  // extern "C"
