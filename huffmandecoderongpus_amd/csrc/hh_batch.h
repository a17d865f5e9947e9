// hh_batch.h -- host interface of the batched decode (hh_batch.hip,
// hh_batch_plan.hip), used by the decoder's entry points (hh_device.hip;
// BatchDev is part of struct hh_decoder, hh_dec.h).  C++ only, not part of
// the public ABI.
#ifndef HH_BATCH_H_
#define HH_BATCH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_fsm_dev.h"
#include "hiphuff.h"

#define HB_UNTOUCHED 0x7fffffff     // a result slot the kernel did not write

// a stream, in the kernel's order; idx: its index in the caller's list
struct BatchDesc {
    uint64_t data_off, bits, out_off, cap, idx;
};
struct BatchRes {
    uint64_t len;
    int64_t status;
};

// The batch launch's shape for the tables in a decoder's FsmDev, and its
// workspace: descriptors and per-stream results on the device, their pinned
// host copies; both grown on demand.
struct BatchDev {
    uint32_t ok;             // k_batch decodes this tree (batch_setup)
    uint32_t W;              // waves per workgroup: tiles per round
    uint32_t G;              // head bits of a guess (hh_fsm_pick_head over the emission step)
    uint32_t minlen;         // shortest code: the staging holds the most symbols a round can have
    uint32_t lds;            // dynamic LDS bytes
    uint32_t grid_max;       // resident workgroups (0: not sized yet)
    void *d_ws, *h_ws;
    size_t d_size, h_size;
    // the last batch of device items (batch_decode_items): not waited for by its call
    hipEvent_t end;          // recorded after its last kernel (0: not created yet)
    int pend;                // 1: recorded and not known to have passed
    hipStream_t pend_st;     // its stream
};

// After the tree's tables are uploaded (fd->ok): the round's shape.
void batch_setup(BatchDev *b, const FsmDev *fd, uint32_t G, uint32_t minlen);
void batch_free(BatchDev *b);
// The host waits for a pending batch of device items (the tables and the
// workspace it uses are about to change).
int batch_wait(BatchDev *b);
// One launch for items[0..n) (validated by the caller), enqueued on st;
// returns when done: out_len[i], status[i] (may be NULL); *ms the launch's
// device time (events ev[0], ev[1]), *lanes the regions of all streams.
// Returns HH_OK or the status of the lowest-index failing stream.
int batch_decode(BatchDev *b, const FsmDev *fd, hipEvent_t *ev, const void *d_data, const hh_batch_item *items,
                 uint64_t n, void *d_out, uint64_t *out_len, int32_t *status, hipStream_t st, float *ms,
                 uint64_t *lanes);
// The same decode from a device list, all of it enqueued on st: the plan
// (items -> checked, bin-ordered descriptors), k_batch, the results into
// d_out_len / d_status / d_summary (may be NULL).  Returns once enqueued.
int batch_decode_items(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                       const hh_batch_item *d_items, uint64_t n, void *d_out, uint64_t out_bytes,
                       uint64_t *d_out_len, int32_t *d_status, hh_batch_summary *d_summary, hipStream_t st);

// hh_batch_plan.hip: the kernels around k_batch of a batch of device items.
// key: a byte per item (hh_batch_plan_algo.h), tmp: the descriptors in index
// order, ctl: HB_PLAN_CTL_BYTES of counters.
#define HB_PLAN_CTL_BYTES 1024u
int batch_plan_enqueue(const hh_batch_item *d_items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                       uint64_t round_bits, BatchDesc *desc, BatchRes *res, BatchDesc *tmp, uint8_t *key,
                       uint32_t *ctl, hh_batch_summary *d_summary, hipStream_t st);
int batch_results_enqueue(const BatchRes *res, const uint8_t *key, uint32_t n, uint64_t *d_out_len,
                          int32_t *d_status, hh_batch_summary *d_summary, uint32_t *ctl, hipStream_t st);
// The empty summary into d_summary, in the order of st.
int batch_summary_clear(hh_batch_summary *d_summary, hipStream_t st);

#endif
