/*
 * hh_batch_plan_algo.h -- the rules of the batched decode's device-side plan
 * (hh_batch_plan.hip: k_plan_count, k_plan_place), __host__ __device__: the
 * kernels run them per item, the test-only emulator
 * (tests/emu/hh_batch_plan_emu.cpp) runs the same functions on the host.
 *
 * hh_decode_batch_device_items takes its items from device memory, so what
 * hh_decode_batch_device checks on the host before anything is launched is
 * checked here, per item, by the kernel that reads the list:
 *
 *   valid   hbp_item_ok: the header's three rules (hiphuff.h, hh_batch_item),
 *           overflow-safe.  An item that breaks one never becomes an address:
 *           its descriptor is hbp's empty one (bits 0, cap 0, offsets 0), for
 *           which k_batch walks no round, loads no payload word and stores no
 *           output byte.
 *   key     hbp_bin: the stream's rounds, ceil(bits / RB) for a round of RB =
 *           64 W S bits, clamped into HBP_BINS bins.  A round is the unit of a
 *           workgroup's time (its lanes walk their regions side by side: a
 *           round costs the same whether 1 or 64 W of them hold bits), so
 *           streams of one bin cost the same and their order is free.
 *   order   the descriptor list by non-increasing bin: bin b's streams start
 *           at hbp_start(b) = the streams of all bins above it.
 *
 * HBP_BINS = 64: one lane per bin in the wave that turns the counts into
 * starts.  Bin 63 holds every stream of 63 rounds or more; among those the
 * order is free too, so a batch's tail may be longer than under an exact
 * sort by at most the spread of their lengths.  63 rounds are 63 x 64 W S
 * bits (kjv's tree, W = 6 and S = 256: 756 KiB of payload, about 1.3 MiB of
 * text): streams of that size take so many rounds each that the resident
 * workgroups (1 to 3 per compute unit) are busy with them for long whatever
 * their order, and the streams below them, which fill the tail, are ordered.
 */
#ifndef HH_BATCH_PLAN_ALGO_H_
#define HH_BATCH_PLAN_ALGO_H_

#include <stdint.h>

#include "hh_fsm_algo.h"
#include "hiphuff.h"

#define HBP_BINS 64u
#define HBP_INVALID 0x80u            /* in an item's key byte: the item broke a rule */

/* The header's rules for one item of a batch over data_bytes of payload and
 * out_bytes of output.  1: the item may be decoded. */
HH_FD int hbp_item_ok(uint64_t data_off, uint64_t bits, uint64_t out_off, uint64_t cap, uint64_t data_bytes,
                      uint64_t out_bytes) {
    if (data_off % 4u) return 0;
    if (bits) {
        const uint64_t nb = bits / 8u + (bits % 8u != 0) + HH_PAYLOAD_PAD;   /* (bits / 8 <= 2^61: no overflow) */
        if (data_off > data_bytes || nb > data_bytes - data_off) return 0;
    }
    if (out_off > out_bytes || cap > out_bytes - out_off) return 0;
    return 1;
}

/* A stream's bin: its rounds of RB > 0 bits, HBP_BINS - 1 for that many or more. */
HH_FD uint32_t hbp_bin(uint64_t bits, uint64_t RB) {
    const uint64_t rounds = bits / RB + (bits % RB != 0);
    return rounds < HBP_BINS - 1u ? (uint32_t)rounds : HBP_BINS - 1u;
}

/* An item's key byte: its bin, or bin 0 | HBP_INVALID. */
HH_FD uint32_t hbp_key(uint64_t data_off, uint64_t bits, uint64_t out_off, uint64_t cap, uint64_t data_bytes,
                       uint64_t out_bytes, uint64_t RB) {
    return hbp_item_ok(data_off, bits, out_off, cap, data_bytes, out_bytes) ? hbp_bin(bits, RB) : HBP_INVALID;
}

/* The first list position of bin b: the streams of the bins above it. */
HH_FD uint32_t hbp_start(const uint32_t *cnt, uint32_t b) {
    uint32_t s = 0;
    for (uint32_t k = b + 1u; k < HBP_BINS; k++) s += cnt[k];
    return s;
}

#endif
