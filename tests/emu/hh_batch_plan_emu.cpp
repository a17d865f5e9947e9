// hh_batch_plan_emu.cpp -- TEST-ONLY host run of the batched decode's
// device-side plan (hh_batch_plan.hip: k_plan_count, k_plan_place) with the
// same rules (hh_batch_plan_algo.h): every item checked and keyed, the
// streams per bin counted workgroup by workgroup, the bins' starts from the
// counts, every workgroup's share of a bin reserved on the bin's cursor and
// its streams placed by their rank in the share -- for any workgroup size and
// for the workgroups arriving at the cursors in either order, so that what
// the atomics leave open is covered without a GPU.  Nothing in the product
// links this file (tests/emu/libhh_emu.so).
#include <stdint.h>

#include <vector>

#include "hh_batch_plan_algo.h"
#include "hiphuff.h"

extern "C" {

uint32_t hh_batch_plan_bins(void) { return HBP_BINS; }

int32_t hh_batch_plan_item_ok(uint64_t data_off, uint64_t bits, uint64_t out_off, uint64_t cap, uint64_t data_bytes,
                              uint64_t out_bytes) {
    return hbp_item_ok(data_off, bits, out_off, cap, data_bytes, out_bytes);
}

uint32_t hh_batch_plan_bin(uint64_t bits, uint64_t round_bits) { return hbp_bin(bits, round_bits); }

// items: n rows of (data_off, bits, out_off, cap).  tb: items per workgroup;
// reverse: the workgroups reach the cursors last first.  key[i]: the item's
// key byte; order[k]: the index of the k-th descriptor; desc: n rows of
// (data_off, bits, out_off, cap, idx), the list k_batch would read.  Returns
// HH_OK, or HH_ERR_INTERNAL when a place is outside the list or taken twice.
int32_t hh_batch_plan_emu(const uint64_t *items, uint64_t n, uint64_t data_bytes, uint64_t out_bytes,
                          uint64_t round_bits, uint32_t tb, int32_t reverse, uint8_t *key, uint32_t *order,
                          uint64_t *desc) {
    if (tb == 0 || round_bits == 0 || n >= 0xffffffffull) return HH_ERR_ARG;
    const uint64_t nwg = (n + tb - 1) / tb;
    std::vector<uint64_t> tmp(5 * n);
    uint32_t cnt[HBP_BINS] = {0}, cur[HBP_BINS] = {0};
    // k_plan_count
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t *it = items + 4 * i;
        const uint32_t k = hbp_key(it[0], it[1], it[2], it[3], data_bytes, out_bytes, round_bits);
        const bool ok = !(k & HBP_INVALID);
        for (int f = 0; f < 4; f++) tmp[5 * i + f] = ok ? it[f] : 0;
        tmp[5 * i + 4] = i;
        key[i] = (uint8_t)k;
        cnt[k & (HBP_BINS - 1u)]++;
    }
    // k_plan_place
    std::vector<uint8_t> taken(n, 0);
    for (uint64_t g = 0; g < nwg; g++) {
        const uint64_t wg = reverse ? nwg - 1 - g : g;
        const uint64_t i0 = wg * tb, i1 = i0 + tb < n ? i0 + tb : n;
        uint32_t loc[HBP_BINS] = {0}, base[HBP_BINS];
        std::vector<uint32_t> rank(i1 - i0);
        for (uint64_t i = i0; i < i1; i++) rank[i - i0] = loc[key[i] & (HBP_BINS - 1u)]++;
        for (uint32_t b = 0; b < HBP_BINS; b++) {
            base[b] = hbp_start(cnt, b) + cur[b];
            cur[b] += loc[b];
        }
        for (uint64_t i = i0; i < i1; i++) {
            const uint64_t at = (uint64_t)base[key[i] & (HBP_BINS - 1u)] + rank[i - i0];
            if (at >= n || taken[at]) return HH_ERR_INTERNAL;
            taken[at] = 1;
            order[at] = (uint32_t)i;
            for (int f = 0; f < 5; f++) desc[5 * at + f] = tmp[5 * i + f];
        }
    }
    return HH_OK;
}

}  // extern "C"
