// hh_enc.h -- the encoder handle, shared by csrc/hh_encode.hip (encode,
// compress), csrc/hh_encb.hip (blocked encode, compress), csrc/hh_encr.hip
// (ragged blocked encode, compress) and csrc/hh_hist.hip (histogram).  Not
// part of the public ABI.
#ifndef HH_ENC_H_
#define HH_ENC_H_

#include <stddef.h>
#include <stdint.h>

// An encoder: the workspace of one device's encodes (the table, the chunks'
// bits / offsets, the total and the absent-symbol flag) and of its
// histograms (the workgroups' partial sums, the 256 counts), kept across
// calls and grown when a call needs more.  Calls on one encoder run one at a
// time (each returns when its work is done); encoders are independent, so
// encodes on several streams run at once with one encoder each.
struct hh_encoder {
    int device;
    uint8_t *ws;
    size_t size;
    uint8_t *hist_ws;       // [rows][256] u32 slab, then 256 u64 counts
    size_t hist_size;
    int cus;                // compute units of the device (0: not asked yet)
    uint64_t *host_bits;    // page-locked: a blocked encode's per-block bits come back here
    size_t host_bits_n;     // (entries)
};

#endif
