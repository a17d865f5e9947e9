// hh_batch.h -- host interface of the batched decode (hh_batch.hip), used by
// the decoder's entry points (hh_device.hip; BatchDev is part of struct
// hh_decoder, hh_dec.h).  C++ only, not part of the public ABI.
#ifndef HH_BATCH_H_
#define HH_BATCH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hh_fsm_dev.h"
#include "hiphuff.h"

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
};

// After the tree's tables are uploaded (fd->ok): the round's shape.
void batch_setup(BatchDev *b, const FsmDev *fd, uint32_t G, uint32_t minlen);
void batch_free(BatchDev *b);
// One launch for items[0..n) (validated by the caller), enqueued on st;
// returns when done: out_len[i], status[i] (may be NULL); *ms the launch's
// device time (events ev[0], ev[1]), *lanes the regions of all streams.
// Returns HH_OK or the status of the lowest-index failing stream.
int batch_decode(BatchDev *b, const FsmDev *fd, hipEvent_t *ev, const void *d_data, const hh_batch_item *items,
                 uint64_t n, void *d_out, uint64_t *out_len, int32_t *status, hipStream_t st, float *ms,
                 uint64_t *lanes);

#endif
