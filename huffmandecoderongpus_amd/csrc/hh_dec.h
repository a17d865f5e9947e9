// hh_dec.h -- what the decoder's host units (hh_device.hip, hh_r2.hip,
// hh_exact.hip, hh_host.hip) share: struct hh_decoder, defined here only, and
// the functions that cross between them.  C++ only, not part of the public ABI.
#ifndef HH_DEC_H_
#define HH_DEC_H_

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include "hh_batch.h"
#include "hh_fsm_dev.h"
#include "hh_internal.h"
#include "hiphuff.h"

#define HH_DBG_WORDS 16             // u64 diagnostic counters (HH_DIAG builds; hh_debug_counters)
#define HH_MAXLEN_FAST 32           // longest code of the fast path (one cursor step <= 32 bits)
// Launch parameters of hh_r2.hip's k_emit that hh_decoder_set_tree reads too
// (the decoder's defaults, the region size of a fixed-length code).
// k_emit's waves per workgroup share one copy of the tables: 16 (one
// workgroup per CU with the 12-bit L1, 32 KiB) when the tables fit beside
// them, else 8 (2 / 4 / 8 waves with the 11-bit L1: emit 3.02 / 2.07 / 1.80
// ms; 16 with the 12-bit L1: 1.43 ms).
#define HH_EMIT_NW_MAX 16
#ifndef HH_XPT
#define HH_XPT 4                    // k_emit: deferred runs per tile a wave's list holds
#endif
#define HH_OBW (4096 + 64)          // k_emit's LDS output staging per wave (bytes): a text tile's
                                    // output (~3.7 K symbols for kjv) plus the 16-B phase

#define HIP_OK(x)                                                             \
    do {                                                                      \
        hipError_t e_ = (x);                                                  \
        if (e_ != hipSuccess) {                                               \
            fprintf(stderr, "hiphuff: %s failed: %s\n", #x, hipGetErrorString(e_)); \
            return HH_ERR_DEVICE;                                             \
        }                                                                     \
    } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct DevTab {
    const uint64_t *l1;
    const uint16_t *f;   // the front's table (hh_internal.h F) and its escape directory
    const uint32_t *fdir;
    uint32_t fdir_used;
    const uint32_t *l2;
    const uint32_t *tree;
    const uint8_t *tsym;
    uint32_t l2_used;
    uint32_t tree_lds;   // compact tree nodes k_emit stages in LDS
};
#define HH_TREE_LDS_MAX 1024   // nodes: a byte alphabet's tree has <= 511 unless symbols repeat;
                               // larger trees take the stage pipeline

struct hh_decoder {
    int device;
    hh_config cfg;
    hipStream_t stream;
    hh_tables *ht;
    int have_tree;
    uint64_t *d_l1;
    uint16_t *d_f;
    uint32_t *d_fdir;
    uint32_t *d_l2;
    uint32_t *d_tree;
    uint8_t *d_tsym;
    DevTab tab;
    uint32_t S;
    uint32_t G;          // overlap bits (hh_pick_overlap; HH_OVERLAP overrides)
    // workspace
    void *ws;
    size_t ws_size;
    uint32_t *h_flags;   // pinned
    int32_t *d_max;      // findmax result (stage API)
    uint64_t *d_dbg;     // HH_DIAG counters (16 x u64)
    hipEvent_t ev[4];
    hipEvent_t ev2[4];         // result slot 1's events (an asynchronous decode behind another)
    hh_stats stats;
    uint32_t grid_f, grid_e, grid_w, grid_x;   // persistent grid sizes (occupancy x CUs)
    uint32_t fwalk;            // k_front's walk bound (HH_FRONT_WALK overrides)
    uint32_t ncu;              // compute units
    uint32_t fixed_len;        // L of a complete fixed-length code (k_fixed), else 0
    uint8_t *d_fsym;           // its 256-entry window -> symbol table
    uint32_t emit_nw;          // k_emit's waves per workgroup (size_grids)
    uint32_t emit_nw_max;      // the largest tried (HH_EMIT_NW = 8 forces the smaller one)
    uint32_t xpt;              // k_emit's deferred runs per tile (HH_EMIT_XPT overrides)
    uint32_t grid_sw;          // words per region they were sized for
    size_t grid_l2;            // and the L2 table size
    uint32_t grid_tree;        // and the LDS tree size
    uint32_t grid_fdir;        // and the F escape directory
    uint32_t grid_nw_max;      // and k_emit's largest workgroup
    // host staging of the evaluate() scope (hh_decode_host)
    uint8_t *h_stage;          // 2 x HH_HOST_CHUNK pinned (hh_decode_host)
    hipEvent_t h_ev[2];
    void *d_in, *d_out;
    size_t d_in_size, d_out_size;
    // the state-machine decode (hh_fsm.hip): tables, device copies, workspace
    hh_fsm_tables *ft;
    FsmDev fsm;
    FsmWs fsm_ws;
    // evaluate() scope pipeline (host_pipeline): copy streams, per-chunk events
    hipStream_t h2d, d2h;
    hipEvent_t *pipe_ev;
    uint32_t npipe_ev;
    // caller buffers kept page-locked across calls (HH_FLAG_KEEP_HOST_PINNED)
    const void *pin_p[2];
    size_t pin_n[2];
    int pin_own[2];      // 1: pin_p[k] registered for buffer k (pages pin_ra..pin_rb); 0: inside k^1's
    uintptr_t pin_ra[2], pin_rb[2];
    // the asynchronous decode not checked yet (hh_decode_device_async)
    struct {
        int active;
        int fixed;             // a k_fixed launch (the length was known at launch)
        FsmPend pd;
        const void *d_data;
        uint64_t bits;
        void *d_out;
        uint64_t *out_len;
        hipStream_t st;
        hh_range_out *ro;      // a segment's decode (hh_decode_device_range_async): its results
    } apend;
    int async_rc;              // the first failure since the last hh_decode_wait
    // the batched decode (hh_batch.hip): its launch shape for the current tree, its workspace
    BatchDev batch;
};

// hh_device.hip
int ensure_dev(void **p, size_t *have, size_t need);   // a kept device buffer, grown to `need`
int fast_path_ok(const hh_decoder *d);
bool fsm_path_ok(const hh_decoder *d);
void fsm_stats(hh_decoder *d, uint64_t bits, uint64_t total, const float *ms, uint32_t one);
int async_check(hh_decoder *d);
// hh_r2.hip
int decode_fast(hh_decoder *d, const void *d_data, uint64_t bits_avail, uint64_t ntiles, uint32_t in_state,
                uint64_t emit_from, void *d_out, uint64_t cap, hipStream_t st, uint64_t *total, uint32_t *leave,
                uint32_t *cst_pro, uint32_t *cst_seg, uint32_t *entry);
// hh_exact.hip
int segment_path(hh_decoder *d, const void *d_data, uint64_t bits, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                 hipStream_t st);
int fixed_path(hh_decoder *d, const void *d_data, uint64_t bits, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
               hipStream_t st, hipEvent_t *ev = nullptr, bool wait = true);
int stage_pipeline(hh_decoder *d, const void *d_data, int64_t bits, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                   hipStream_t st);

#endif
