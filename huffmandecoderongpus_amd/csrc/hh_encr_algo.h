// hh_encr_algo.h -- the rules of the ragged blocked encode (records cut at an
// offsets list; csrc/hh_encr.hip), host and device: what the kernels run and
// what tests/emu/hh_encr_emu.cpp runs chunk by chunk on the CPU.
//
// offs: nrec + 1 values, offs[0] == 0, nondecreasing, offs[nrec] == n; record
// r is the symbols [offs[r], offs[r + 1]).  P(i): the exclusive prefix of the
// code lengths over all n symbols.  start[r] = P(offs[r]); bits[r] =
// start[r + 1] - start[r]; wb[r], the record's first output word, the
// exclusive prefix of ceil(bits / 32).
#ifndef HH_ENCR_ALGO_H_
#define HH_ENCR_ALGO_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define HER_FN __host__ __device__ static inline
#else
#define HER_FN static inline
#endif

#define HER_CH 4096u                // symbols per chunk (ENC_CH)
#define HER_TILE 1024u              // entries per scan tile (ENC_SCAN_TB)
#define HER_F_ABSENT 1u             // flag word: a symbol absent from the tree
#define HER_F_OFFS 2u               //            offs breaks one of its rules
#define HER_F_INTERNAL 4u           //            a bound check inside a kernel

// The first r in [0, nrec) with offs[r] >= target, nrec if there is none: the
// records that start in the symbols [a, b) are those in [lower(a), lower(b)).
// In range whatever offs holds.
HER_FN uint64_t her_lower(const uint64_t *offs, uint64_t nrec, uint64_t target) {
    uint64_t lo = 0, hi = nrec;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offs[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The record of symbol i < n: the upper bound of i in offs, minus 1 -- the
// last r with offs[r] <= i, which skips the empty records at that offset.
HER_FN uint64_t her_record_of(const uint64_t *offs, uint64_t nrec, uint64_t i) {
    uint64_t lo = 0, hi = nrec + 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offs[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// The offsets check of one pair (a = offs[r], b = offs[r + 1]): nondecreasing
// and within the text; with offs[0] == 0 and offs[nrec] == n, all the rules.
HER_FN int her_pair_ok(uint64_t a, uint64_t b, uint64_t n) { return a <= b && b <= n; }

// start[r] from the chunks' exclusive bit offsets CS (CS[c] = P(c HER_CH)) and
// loc[r], the bits of the chunk before symbol offs[r]; the total for a record
// at the text's end.  o <= n.
HER_FN uint64_t her_start(const uint64_t *CS, uint64_t o, uint32_t loc, uint64_t n, uint64_t total) {
    return o == n ? total : CS[o / HER_CH] + loc;
}

HER_FN uint64_t her_words(uint64_t bits) { return (bits + 31) / 32; }

// The position formula: the output bit of a symbol of record r whose prefix
// is P.
HER_FN uint64_t her_pos(uint64_t wb, uint64_t start, uint64_t P) { return 32 * wb + (P - start); }

// A chunk's image: the output words from that of its first symbol's first bit
// (g0) to that of its last symbol's last bit (gend, exclusive, > g0).
HER_FN uint64_t her_img_words(uint64_t g0, uint64_t gend) { return (gend + 31) / 32 - g0 / 32; }

// Words that hold any chunk's image: its first bit anywhere in a word, HER_CH
// codes of at most maxlen bits, up to 31 bits of padding at every record
// start inside the chunk (at most HER_CH - 1 of them, and fewer than nrec),
// the round-up.
HER_FN uint32_t her_img_alloc(uint32_t maxlen, uint64_t nrec) {
    const uint32_t starts = nrec < HER_CH ? (uint32_t)nrec : HER_CH;
    return (31u + HER_CH * maxlen + 31u * starts + 31u) / 32u + 1u;
}

#endif
