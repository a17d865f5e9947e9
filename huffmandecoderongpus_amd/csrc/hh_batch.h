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

// a stream, in the kernel's order; idx: its index in the caller's list.
// win != 0: a window piece (hh_decode_blocks_read) -- of the stream's symbols
// only [skip, skip + cap) are wanted, at out_off; the result's len is the
// bytes delivered.  win == 0 (skip 0): a whole stream clipped to cap.
struct BatchDesc {
    uint64_t data_off, bits, out_off, cap, idx, skip;
    uint32_t win, pad;
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
    // the record take's kernel (hh_batch_take.hip): its resident workgroups for tk_W waves and tk_lds bytes
    uint32_t tk_W, tk_lds, tk_grid;
};

// What a round's kernels share (k_batch, hh_batch.hip; k_gather,
// hh_batch_gather.hip): the LDS they may use, the round's geometry and the
// emission sink.
#define HB_LDS (160u * 1024u)

struct BatchGeo {
    uint32_t ns, K, r, S, G, W;
    uint32_t pay_off, misc_off, stg_off, stg_bytes;   // LDS byte offsets / the staging's size
    uint32_t n;
};

// The emission sink: a step's symbols shifted into the current dword, which
// is stored to its aligned staging address once its last byte is there (the
// bytes of earlier runs in it zero); a run that ends inside a dword ORs its
// bytes in after every run's stores (k_emf's scheme, hh_fsm.hip).
struct BatchSink {
    uint8_t *lds;
    uint32_t wd, sh, a;
    __device__ __forceinline__ void init(uint8_t *smem, uint32_t oa) {
        lds = smem;
        wd = oa & ~3u;
        sh = (oa & 3u) * 8u;
        a = 0;
    }
    __host__ __device__ __forceinline__ void put(uint64_t e) {
        const uint32_t lo = (uint32_t)e, u = sh + ((uint32_t)(e >> 32) & 255u);
        const uint64_t t = (uint64_t)lo << sh;
        const uint32_t an = (uint32_t)t | a;
        const bool full = u >= 32u;
        if (full) *(uint32_t *)(lds + wd) = an;
        a = full ? (uint32_t)(t >> 32) : an;
        wd += full ? 4u : 0u;
        sh = u & 31u;
    }
};

// After the tree's tables are uploaded (fd->ok): the round's shape.
void batch_setup(BatchDev *b, const FsmDev *fd, uint32_t G, uint32_t minlen);
void batch_free(BatchDev *b);
// The host waits for a pending batch of device items (the tables and the
// workspace it uses are about to change).
int batch_wait(BatchDev *b);
// The workspace grown to need_d device and need_h pinned host bytes; the
// geometry of a launch over n list entries.
int batch_ws(BatchDev *b, size_t need_d, size_t need_h);
BatchGeo batch_geo(const BatchDev *b, const FsmDev *fd, uint64_t n);
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

// Range reads over a blocked buffer (hh_decode_blocks_read), all of it
// enqueued on st: the plan (reads -> window pieces, hh_batch_read.hip), the
// bin order, k_batch over the P slots of the piece budget, the gather of the
// pieces' results into d_read_len / d_status / d_summary (may be NULL).
int batch_decode_read(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                      const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms, const hh_block_read *d_reads,
                      uint64_t m, uint32_t P, void *d_out, uint64_t out_bytes, uint64_t *d_read_len,
                      int32_t *d_status, hh_batch_summary *d_summary, hipStream_t st);

// hh_batch_plan.hip: the kernels around k_batch of a batch of device items.
// key: a byte per item (hh_batch_plan_algo.h), tmp: the descriptors in index
// order, ctl: HB_PLAN_CTL_BYTES of counters.
#define HB_PLAN_CTL_BYTES 1024u
// ctl's u32 words: the streams per bin, the bins' placement cursors, the
// results' workgroups finished; for range reads the slots that hold a piece
// and (two words, 8-byte aligned) the first failing read << 32 | -status
#define HB_CTL_CNT 0u
#define HB_CTL_CUR 64u
#define HB_CTL_DONE 128u
#define HB_CTL_TOTAL 130u
#define HB_CTL_FIRST 132u
// for gathered reads (hh_batch_gather.hip): the walks, i.e. the touched blocks
#define HB_CTL_WALKS 134u
int batch_plan_enqueue(const hh_batch_item *d_items, uint32_t n, uint64_t data_bytes, uint64_t out_bytes,
                       uint64_t round_bits, BatchDesc *desc, BatchRes *res, BatchDesc *tmp, uint8_t *key,
                       uint32_t *ctl, hh_batch_summary *d_summary, hipStream_t st);
int batch_results_enqueue(const BatchRes *res, const uint8_t *key, uint32_t n, uint64_t *d_out_len,
                          int32_t *d_status, hh_batch_summary *d_summary, uint32_t *ctl, hipStream_t st);
// k_plan_place alone: tmp[0..n) by their key bytes into desc; ctl's counts
// per bin are the caller's (batch_plan_enqueue's k_plan_count, or the range
// reads' k_read_fill).
int batch_place_enqueue(const BatchDesc *tmp, const uint8_t *key, uint32_t n, uint32_t *ctl, BatchDesc *desc,
                        hipStream_t st);
// The empty summary into d_summary, in the order of st.
int batch_summary_clear(hh_batch_summary *d_summary, hipStream_t st);


// hh_batch_read.hip: the plan of a range read and the gather of its results.
// The workspace beside desc / res / tmp / key / ctl (which are the items
// batch's, for P slots): per slot the owning read, per read its first slot,
// its copy, its record and its own status.
struct ReadWs {
    BatchDesc *desc, *tmp;
    BatchRes *res;
    uint64_t *start;         // m: a read's piece count, then (k_read_scan) its first slot
    hh_block_read *reads;    // m: the caller's list, copied by the one kernel that reads it
    uint64_t *rec;           // 2 m: delivered bytes; min over failing pieces of (block ordinal << 8 | -status)
    uint32_t *own;           // P: a slot's read
    int32_t *rstat;          // m: HH_ERR_ARG for a read that gets no piece, else HH_OK
    uint32_t *ctl;
    uint8_t *key;
};
size_t read_ws_bytes(uint64_t m, uint32_t P);
void read_ws_carve(ReadWs *w, void *d_ws, uint64_t m, uint32_t P);
int read_plan_enqueue(const ReadWs *w, const hh_batch_item *d_index, uint64_t data_bytes, uint64_t n_syms,
                      uint64_t block_syms, const hh_block_read *d_reads, uint32_t m, uint32_t P, uint64_t out_bytes,
                      uint64_t round_bits, hh_batch_summary *d_summary, hipStream_t st);
int read_results_enqueue(const ReadWs *w, uint32_t m, uint32_t P, uint64_t *d_read_len, int32_t *d_status,
                         hh_batch_summary *d_summary, hipStream_t st);
// The plan's first half alone (the counters cleared, k_read_count,
// k_read_scan): validity, first slots, the slots that hold a piece.
int read_count_enqueue(const ReadWs *w, uint64_t n_syms, uint64_t block_syms, const hh_block_read *d_reads,
                       uint32_t m, uint32_t P, uint64_t out_bytes, hh_batch_summary *d_summary, hipStream_t st);

// hh_batch_gather.hip: gathered range reads (hh_decode_blocks_gather) -- the
// plan of hh_decode_blocks_read up to the pieces, the pieces grouped by block
// and k_gather, which walks every touched block once for all its pieces.
// nb: the blocks of the buffer (< 2^32 - 1, hbg_blocks).
int batch_decode_gather(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                        const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms,
                        const hh_block_read *d_reads, uint64_t m, uint32_t P, uint32_t nb, void *d_out,
                        uint64_t out_bytes, uint64_t *d_read_len, int32_t *d_status, hh_batch_summary *d_summary,
                        hipStream_t st);

// hh_batch_take.hip: the record take (hh_decode_batch_take) -- the plan over
// the taken records, k_take's packed rounds, the summary; all enqueued on st.
// batch_take_waves: k_take's waves per workgroup and LDS bytes for the tree.
int batch_decode_take(BatchDev *b, const FsmDev *fd, const void *d_data, uint64_t data_bytes,
                      const hh_batch_item *d_index, uint64_t nrec, const uint64_t *d_ids, uint64_t m, void *d_out,
                      uint64_t out_bytes, uint64_t *d_out_offs, int32_t *d_status, hh_batch_summary *d_summary,
                      hipStream_t st);
int batch_take_waves(const BatchDev *b, const FsmDev *fd, uint32_t *W, uint32_t *lds);

#endif
