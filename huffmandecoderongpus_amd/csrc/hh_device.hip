// hh_device.hip -- the decoder object and the device half of the C ABI: create,
// destroy, set_tree, and the decode entry points, which pick a path (hh_fsm.hip,
// hh_one.hip, hh_batch.hip, hh_r2.hip, hh_exact.hip).  No kernels here.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hh_algo.h"
#include "hh_batch_gather_algo.h"
#include "hh_batch_read_algo.h"
#include "hh_dec.h"
#include "hh_fsm_algo.h"
#include "hh_internal.h"
#include "hiphuff.h"

int ensure_dev(void **p, size_t *have, size_t need) {
    if (*have >= need) return HH_OK;
    if (*p) HIP_OK(hipFree(*p));
    *p = nullptr;
    *have = 0;
    const size_t sz = need + need / 8;
    if (hipMalloc(p, sz) != hipSuccess) return HH_ERR_NOMEM;
    *have = sz;
    return HH_OK;
}

extern "C" int hh_decoder_create(hh_decoder **out, const hh_config *cfg) {
    if (!out) return HH_ERR_ARG;
    *out = nullptr;
    hh_decoder *d = (hh_decoder *)calloc(1, sizeof(hh_decoder));
    if (!d) return HH_ERR_NOMEM;
    if (cfg) d->cfg = *cfg;
    d->device = d->cfg.device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || d->device < 0 || d->device >= ndev) {
        free(d);
        return HH_ERR_DEVICE;
    }
    if (hipSetDevice(d->device) != hipSuccess) { free(d); return HH_ERR_DEVICE; }
    d->ht = (hh_tables *)calloc(1, sizeof(hh_tables));
    d->ft = (hh_fsm_tables *)calloc(1, sizeof(hh_fsm_tables));
    if (!d->ht || !d->ft) { free(d->ht); free(d->ft); free(d); return HH_ERR_NOMEM; }
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&d->d_l1, sizeof(uint64_t) * HH_L1_SIZE) != hipSuccess ||
        hipMalloc(&d->d_l2, sizeof(uint32_t) * HH_L2_MAX) != hipSuccess ||
        hipMalloc(&d->d_f, sizeof(uint16_t) * HH_F_SIZE) != hipSuccess ||
        hipMalloc(&d->d_fdir, sizeof(uint32_t) * HH_L2_MAX) != hipSuccess ||
        hipMalloc(&d->d_fsym, 256) != hipSuccess ||
        hipMalloc(&d->d_tree, sizeof(uint32_t) * (HH_TREE_MAX + 1)) != hipSuccess ||
        hipMalloc(&d->d_tsym, HH_TREE_MAX + 1) != hipSuccess ||
        hipMalloc(&d->d_max, 16) != hipSuccess ||
        hipMalloc(&d->d_dbg, HH_DBG_WORDS * sizeof(uint64_t)) != hipSuccess ||
        hipHostMalloc((void **)&d->h_flags, 64, hipHostMallocDefault) != hipSuccess) {
        hh_decoder_destroy(d);
        return HH_ERR_DEVICE;
    }
    for (int i = 0; i < 4; i++) {
        if (hipEventCreate(&d->ev[i]) != hipSuccess || hipEventCreate(&d->ev2[i]) != hipSuccess) {
            hh_decoder_destroy(d);
            return HH_ERR_DEVICE;
        }
    }
    *out = d;
    return HH_OK;
}

extern "C" void hh_decoder_destroy(hh_decoder *d) {
    if (!d) return;
    hipSetDevice(d->device);
    async_check(d);                     // (an asynchronous decode still running)
    (void)batch_wait(&d->batch);        // (a batch of device items still running)
    hh_decoder_release_host(d);
    if (d->ws) hipFree(d->ws);
    if (d->d_l1) hipFree(d->d_l1);
    if (d->d_l2) hipFree(d->d_l2);
    if (d->d_f) hipFree(d->d_f);
    if (d->d_fdir) hipFree(d->d_fdir);
    if (d->d_fsym) hipFree(d->d_fsym);
    if (d->d_tree) hipFree(d->d_tree);
    if (d->d_tsym) hipFree(d->d_tsym);
    if (d->d_max) hipFree(d->d_max);
    if (d->d_dbg) hipFree(d->d_dbg);
    if (d->d_in) hipFree(d->d_in);
    if (d->d_out) hipFree(d->d_out);
    if (d->h_stage) {
        hipHostFree(d->h_stage);
        hipEventDestroy(d->h_ev[0]);
        hipEventDestroy(d->h_ev[1]);
    }
    if (d->h_flags) hipHostFree(d->h_flags);
    for (int i = 0; i < 4; i++) {
        if (d->ev[i]) hipEventDestroy(d->ev[i]);
        if (d->ev2[i]) hipEventDestroy(d->ev2[i]);
    }
    if (d->stream) hipStreamDestroy(d->stream);
    fsm_free(&d->fsm);
    fsm_ws_free(&d->fsm_ws);
    batch_free(&d->batch);
    for (uint32_t i = 0; i < d->npipe_ev; i++) hipEventDestroy(d->pipe_ev[i]);
    free(d->pipe_ev);
    if (d->h2d) hipStreamDestroy(d->h2d);
    if (d->d2h) hipStreamDestroy(d->d2h);
    free(d->ht);
    free(d->ft);
    free(d);
}

static uint32_t pick_region_bits(const hh_tables *t, int req) {
    uint32_t g = (uint32_t)(t->len_gcd > 0 ? t->len_gcd : 1);
    if (req > 0) {
        // a requested size must keep whole words; off the code lattice it is
        // still exact (walks that cannot merge report failure), only slower
        if (req % 32 || req > 32 * HH_SW_MAX) return 0;
        return (uint32_t)req;
    }
    uint32_t S = hh_pick_region_bits(g);
    // A fixed-length code puts HH_NR * S / len symbols in every tile: keep
    // that within k_emit's staging buffer (E.coli: 2-bit codes, S = 128).
    if (t->fixed_len > 0 && S) {
        uint32_t x = 32, y = g;
        while (y) { const uint32_t r = x % y; x = y; y = r; }
        const uint32_t lcm = 32 / x * g;
        const uint64_t smax = (uint64_t)(HH_OBW - 64) * (uint32_t)t->fixed_len / HH_NR;
        while (S > smax && S > lcm) S -= lcm;
    }
    return S;
}

extern "C" int hh_decoder_set_tree(hh_decoder *d, const hh_tree *tree) {
    if (!d || !tree) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);                     // (a pending asynchronous decode uses the current tables)
    int rc = batch_wait(&d->batch);     // (and so does a batch of device items)
    if (rc) return rc;
    rc = hh_tables_build(tree, d->ht);
    if (rc) return rc;
    HIP_OK(hipSetDevice(d->device));
    HIP_OK(hipMemcpy(d->d_l1, d->ht->l1, sizeof(uint64_t) * HH_L1_SIZE, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->d_l2, d->ht->l2, sizeof(uint32_t) * HH_L2_MAX, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->d_tree, d->ht->tree, sizeof(uint32_t) * (HH_TREE_MAX + 1), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->d_tsym, d->ht->tsym, HH_TREE_MAX + 1, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->d_f, d->ht->f, sizeof(d->ht->f), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d->d_fdir, d->ht->fdir, sizeof(uint32_t) * (d->ht->fdir_used ? d->ht->fdir_used : 1), hipMemcpyHostToDevice));
    d->tab.f = d->d_f;
    d->tab.fdir = d->d_fdir;
    d->tab.fdir_used = d->ht->fdir_used;
    d->tab.l1 = d->d_l1;
    d->tab.l2 = d->d_l2;
    d->tab.tree = d->d_tree;
    d->tab.tsym = d->d_tsym;
    d->tab.l2_used = d->ht->l2_used;
    d->tab.tree_lds = d->ht->tree_used;
    d->S = pick_region_bits(d->ht, d->cfg.lane_bits);
    // trees of more than 127 states: the state machine counts in 7-bit steps
    // over 224-bit regions (hh_fsm.h), and the decoder's tiles are its tiles
    // (tile_bits, shards, the evaluate() chunks)
    if (!(d->cfg.flags & HH_FLAG_LEGACY) && d->cfg.lane_bits == 0) {
        const uint32_t Sf = hh_fsm_region_bits(hh_fsm_nstates(d->ht), (uint32_t)d->ht->len_gcd, d->S);
        if (Sf) d->S = Sf;
    }
    // a complete fixed-length code: every L-bit window is one symbol
    d->fixed_len = 0;
    const int L = d->ht->fixed_len;
    if (L >= 1 && L <= 8 && d->ht->tree_used == (2u << L) - 1u) {
        uint8_t fs[256];
        for (uint32_t w = 0; w < 256; w++) {
            uint32_t node = 0;
            for (int b = 0; b < L; b++) {
                const uint32_t tn = d->ht->tree[node];
                node = (w >> b) & 1u ? (tn >> 15) & 0x7fffu : tn & 0x7fffu;
            }
            fs[w] = (uint8_t)(d->ht->tree[node] & 0xffu);
        }
        HIP_OK(hipMemcpy(d->d_fsym, fs, 256, hipMemcpyHostToDevice));
        d->fixed_len = (uint32_t)L;
    }
    d->fwalk = HH_FRONT_WALK;
    const char *fw = getenv("HH_FRONT_WALK");            // experiments, tests
    if (fw && *fw) d->fwalk = (uint32_t)atoi(fw);
    d->xpt = HH_XPT;
    d->emit_nw_max = HH_EMIT_NW_MAX;
    const char *enw = getenv("HH_EMIT_NW");
    if (enw && atoi(enw) == 8) d->emit_nw_max = 8;
    const char *xp = getenv("HH_EMIT_XPT");
    if (xp && *xp) d->xpt = (uint32_t)atoi(xp);
    d->G = hh_pick_overlap(d->ht);
    if (getenv("HH_OVERLAP")) d->G = (uint32_t)atoi(getenv("HH_OVERLAP")) & ~31u;   // experiments
    if (d->G > HH_GMAX || d->G + 32 > d->S) d->G = 0;
    // the state machine (trees of at most HH_FSM_MAXS = 255 internal nodes)
    fsm_free(&d->fsm);
    // emission steps of 7 bits when their tables leave room for 16 stagings
    // of the expected tile output (fsm_k_fits), else 6 or 5 (smaller tables,
    // more waves), 6 when none does; HH_FSM_K: experiments.  Expected bits per symbol: the code lengths weighted by
    // 2^-length (exact for a code built from a dyadic distribution).
    double avg = 0.0;
    {
        uint32_t stk[64], dep[64], sp = 0;
        stk[sp] = 0; dep[sp++] = 0;
        while (sp) {
            const uint32_t id = stk[--sp], dd = dep[sp];
            const uint32_t e = d->ht->tree[id];
            if ((e & HH_T_LEAF) || dd >= 62) { avg += dd * ldexp(1.0, -(int)dd); continue; }
            stk[sp] = e & 0x7fffu; dep[sp++] = dd + 1;
            stk[sp] = (e >> 15) & 0x7fffu; dep[sp++] = dd + 1;
        }
    }
    const uint32_t est = avg > 0.0 ? (uint32_t)(64.0 * d->S / avg) : 64u * d->S;
    uint32_t Kf = getenv("HH_FSM_K") ? (uint32_t)atoi(getenv("HH_FSM_K")) : 0u;
    // the widest step whose tables leave room for 16 stagings: kjv-like
    // alphabets 7; a byte alphabet (255 states, at most 6) 5 -- its 6-bit
    // tables leave room for 6 waves' stagings (emit 1.07 -> 0.97 ms per GiB)
    for (uint32_t k = 7; !Kf && d->S && k >= 5; k--)
        if (hh_fsm_build(d->ht, d->S, k, d->ft) == HH_OK && d->ft->K == k && fsm_k_fits(d->ft, est)) Kf = k;
    if (d->S && hh_fsm_build(d->ht, d->S, Kf ? Kf : 6, d->ft) == HH_OK) {
        uint32_t Gf = hh_fsm_pick_head(d->ht, d->S, d->ft->cb);
        if (getenv("HH_FSM_HEAD")) Gf = (uint32_t)atoi(getenv("HH_FSM_HEAD")) / d->ft->cb * d->ft->cb;   // experiments
        if (Gf > d->S) Gf = 0;
        const int urc = fsm_upload(&d->fsm, d->ft, Gf, (uint32_t)d->ht->minlen, (uint32_t)d->ht->maxlen);
        d->fsm.dbg = d->d_dbg;
        d->fsm.phases = (d->cfg.flags & HH_FLAG_PHASE_TIMING) != 0;
        d->fsm.two_pass = (d->cfg.flags & HH_FLAG_TWO_PASS) != 0;
        if (urc != HH_OK && urc != HH_ERR_UNSUPPORTED) return urc;
        // the single pass (hh_one.hip): its head over the emission table's
        // K-bit steps, on the code lattice like the count pass's
        uint32_t G1 = hh_fsm_pick_head(d->ht, d->S, d->ft->K);
        if (getenv("HH_FSM_HEAD")) G1 = (uint32_t)atoi(getenv("HH_FSM_HEAD")) / d->ft->K * d->ft->K;   // experiments
        if (urc == HH_OK) one_setup(&d->fsm, G1 > d->S ? 0u : G1, avg, (uint32_t)d->ht->minlen);
    }
    // the batched decode (hh_batch.hip) walks the emission tables only: its
    // head on their K-bit steps too
    {
        const uint32_t Gb = d->fsm.ok ? hh_fsm_pick_head(d->ht, d->S, d->fsm.K) : 0u;
        batch_setup(&d->batch, &d->fsm, Gb > d->S ? 0u : Gb, (uint32_t)d->ht->minlen);
    }
    d->have_tree = 1;
    return HH_OK;
}

extern "C" int hh_decoder_stats(const hh_decoder *d, hh_stats *st) {
    if (!d || !st) return HH_ERR_ARG;
    *st = d->stats;
    return HH_OK;
}

int fast_path_ok(const hh_decoder *d) {
    return d->S >= 32 && d->S <= 32 * HH_SW_MAX && d->ht->maxlen <= HH_MAXLEN_FAST &&
           d->ht->tree_used <= HH_TREE_LDS_MAX && !(d->cfg.flags & (HH_FLAG_FORCE_EXACT | HH_FLAG_FORCE_SEGMENT));
}

// The state-machine path (hh_fsm.hip) decodes whenever its tables exist
// (trees of at most HH_FSM_MAXS internal nodes) and no other path is forced.
bool fsm_path_ok(const hh_decoder *d) {
    return d->fsm.ok && !(d->cfg.flags & (HH_FLAG_LEGACY | HH_FLAG_FORCE_EXACT | HH_FLAG_FORCE_SEGMENT));
}
// ms: count, scan, emission (HH_FLAG_PHASE_TIMING; else 0), total
void fsm_stats(hh_decoder *d, uint64_t bits, uint64_t total, const float *ms, uint32_t one) {
    d->stats.ms_sync = ms[0];
    d->stats.ms_scan = ms[1];
    d->stats.ms_emit = ms[2];
    d->stats.ms_total = ms[3];
    d->stats.lanes = (bits + d->S - 1) / d->S;
    d->stats.out_len = total;
    d->stats.state_machine = one ? 2 : 1;
}

// What every device decode entry point asks of its arguments (nbits: the
// readable stream bits at d_data).
static bool decode_args_ok(const hh_decoder *d, const void *d_data, uint64_t nbits, const void *d_out, uint64_t cap) {
    if (!d || (!d_data && nbits) || (!d_out && cap)) return false;
    if (!d->have_tree) return false;
    return ((uintptr_t)d_data & 3u) == 0;   // word loads
}

// A complete fixed-length code decodes with k_fixed unless another path is forced.
static bool fixed_code_path(const hh_decoder *d) {
    return d->fixed_len && !(d->cfg.flags & (HH_FLAG_NO_FIXED | HH_FLAG_FORCE_EXACT | HH_FLAG_FORCE_SEGMENT));
}

// The exact decode of a stream the chain decodes do not take: the segment
// path for codes of at most HH_MAXLEN_FAST bits, else the stage pipeline.
static int exact_fallback(hh_decoder *d, const void *d_data, uint64_t bits, void *d_out, uint64_t cap,
                          uint64_t *out_len, hipStream_t st) {
    const bool seg_ok = d->ht->maxlen <= HH_MAXLEN_FAST && !(d->cfg.flags & HH_FLAG_FORCE_EXACT);
    d->stats.exact_fallback = seg_ok ? 2 : 1;
    if (seg_ok) return segment_path(d, d_data, bits, (uint8_t *)d_out, cap, out_len, st);
    return stage_pipeline(d, d_data, (int64_t)bits, (uint8_t *)d_out, cap, out_len, st);
}

extern "C" int hh_decode_device(hh_decoder *d, const void *d_data, uint64_t bits, void *d_out,
                                uint64_t cap, uint64_t *out_len, void *hip_stream) {
    if (!out_len || !decode_args_ok(d, d_data, bits, d_out, cap)) return HH_ERR_ARG;
    // NULL is the default stream (ordered with the caller's default-stream
    // work, e.g. torch's), never the decoder's private non-blocking stream
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);                     // (an asynchronous decode before it: its status is kept for hh_decode_wait)
    memset(&d->stats, 0, sizeof(d->stats));
    *out_len = 0;
    if (bits == 0) return HH_OK;
    if (fixed_code_path(d)) return fixed_path(d, d_data, bits, (uint8_t *)d_out, cap, out_len, st);
    if (fsm_path_ok(d)) {
        uint64_t total = 0;
        uint32_t leave = 0, en = 0;
        float ms[4] = {0, 0, 0, 0};
        const int rc = fsm_decode(&d->fsm, &d->fsm_ws, d->ev, d_data, bits, 0, 0, 0, d_out, cap, st, &total, &leave,
                                  &en, ms);
        fsm_stats(d, bits, total, ms, d->fsm_ws.last_one);
        if (rc == HH_NOSYNC) {
            // chains that did not meet within HH_FSM_KM regions: a code that
            // does not resynchronise
            d->stats.repairs = 1;
            return exact_fallback(d, d_data, bits, d_out, cap, out_len, st);
        }
        *out_len = total;
        return rc;
    }
    if (!fast_path_ok(d) || (d->cfg.flags & HH_FLAG_FORCE_SEGMENT))
        return exact_fallback(d, d_data, bits, d_out, cap, out_len, st);
    uint64_t total = 0;
    uint32_t leave = 0, cp = 0, cs = 0, en = 0;
    int rc = decode_fast(d, d_data, bits, 0, hh_state_pack(0, 0, 0), 0, d_out, cap, st, &total,
                         &leave, &cp, &cs, &en);
    if (rc == HH_NOSYNC) {
        // A walk found no shared boundary within HH_KM regions (a code that
        // does not resynchronise): the segment path (fast_path_ok: its codes
        // are short enough), exact and O(N).
        d->stats.repairs = 1;
        return exact_fallback(d, d_data, bits, d_out, cap, out_len, st);
    }
    *out_len = total;
    return rc;
}

// ---------------------------------------------------------------------------
// Asynchronous decodes (hh_decode_device_async / hh_decode_wait): a decode is
// enqueued and the PREVIOUS one checked, so that the GPU has the next decode
// queued while the host reads the last one's results (from its own result
// slot and event set: the two alternate).
// ---------------------------------------------------------------------------
static hipEvent_t *slot_ev(hh_decoder *d, uint32_t slot) { return slot ? d->ev2 : d->ev; }

// The first failure since the last hh_decode_wait is the one it reports.
static void async_note(hh_decoder *d, int rc) {
    if (rc != HH_OK && d->async_rc == HH_OK) d->async_rc = rc;
}

// Check the pending asynchronous decode: its length to *out_len, its status
// kept in async_rc (the first failure).  A stream that did not resynchronise
// is decoded again here, on the exact path, as hh_decode_device would.
int async_check(hh_decoder *d) {
    if (!d->apend.active) return HH_OK;
    d->apend.active = 0;
    hipEvent_t *ev = slot_ev(d, d->apend.pd.slot);
    int rc;
    memset(&d->stats, 0, sizeof(d->stats));
    if (d->apend.fixed) {
        rc = hipEventSynchronize(ev[3]) == hipSuccess ? HH_OK : HH_ERR_DEVICE;
        float ms = 0;
        hipEventElapsedTime(&ms, ev[0], ev[3]);
        d->stats.ms_emit = d->stats.ms_total = ms;
        d->stats.fixed_length = 1;
        d->stats.out_len = *d->apend.out_len;
    } else {
        uint64_t total = 0;
        uint32_t leave = 0, en = 0;
        float ms[4] = {0, 0, 0, 0};
        rc = fsm_collect(&d->fsm_ws, ev, &d->apend.pd, &total, &leave, &en, ms);
        uint32_t one = d->apend.pd.one;
        if (rc == HH_ONE_RETRY) {
            // the single pass handed the decode back: the two passes decode
            // it again, synchronously, on the decode's stream
            FsmPend p2;
            memset(&p2, 0, sizeof(p2));
            rc = fsm_launch(&d->fsm, &d->fsm_ws, d->apend.pd.slot, ev, d->apend.d_data, d->apend.bits,
                            d->apend.pd.nt_arg, d->apend.pd.in_state, d->apend.pd.emit_from, d->apend.d_out,
                            d->apend.pd.cap, d->apend.st, &p2, true);
            if (rc == HH_OK) rc = fsm_collect(&d->fsm_ws, ev, &p2, &total, &leave, &en, ms);
            one = 0;
        }
        fsm_stats(d, d->apend.bits, total, ms, one);
        *d->apend.out_len = total;
        if (d->apend.ro) {
            // a segment: its states; one that does not resynchronise is
            // unsupported (decode such a code whole), as the synchronous call
            d->apend.ro->leave_state = leave;
            d->apend.ro->entry_state = en;
            if (rc == HH_NOSYNC) rc = HH_ERR_UNSUPPORTED;
        } else if (rc == HH_NOSYNC) {
            d->stats.repairs = 1;
            rc = exact_fallback(d, d->apend.d_data, d->apend.bits, d->apend.d_out, d->apend.pd.cap, d->apend.out_len,
                                d->apend.st);
        }
    }
    async_note(d, rc);
    return rc;
}

// Enqueue one decode -- k_fixed when `fixed`, else the state machine over
// tiles [0, ntiles) entered in in_state, the first emit_from a prologue --
// into the free result slot, check the previous decode while this one runs,
// and keep this one as pending (ro: a segment's results, else NULL).  Returns
// the launch's status, noted in async_rc; after a failed launch nothing is
// pending.
static int async_enqueue(hh_decoder *d, bool fixed, const void *d_data, uint64_t bits, uint64_t ntiles,
                         uint32_t in_state, uint64_t emit_from, void *d_out, uint64_t cap, uint64_t *out_len,
                         hh_range_out *ro, hipStream_t st) {
    // the previous decode's slot and events stay untouched until it is checked
    const uint32_t slot = d->apend.active ? (d->apend.pd.slot ^ 1u) : 0u;
    FsmPend pd;
    memset(&pd, 0, sizeof(pd));
    pd.slot = slot;
    int rc;
    if (fixed) {
        rc = fixed_path(d, d_data, bits, (uint8_t *)d_out, cap, out_len, st, slot_ev(d, slot), false);
    } else {
        // The state-machine workspace (records, tile sums, corrections) is
        // one per decoder: a decode queued on another stream than the
        // pending one waits for that one's last kernel before its count pass
        // may overwrite what the pending emission still reads.  (On one
        // stream the order is the stream's.)
        if (d->apend.active && !d->apend.fixed && d->apend.st != st)
            HIP_OK(hipStreamWaitEvent(st, slot_ev(d, d->apend.pd.slot)[3], 0));
        rc = fsm_launch(&d->fsm, &d->fsm_ws, slot, slot_ev(d, slot), d_data, bits, ntiles, in_state, emit_from, d_out,
                        cap, st, &pd);
    }
    async_check(d);                     // the previous decode, while this one runs
    async_note(d, rc);
    if (rc != HH_OK) return rc;
    d->apend.active = 1;
    d->apend.fixed = fixed;
    d->apend.pd = pd;
    d->apend.d_data = d_data;
    d->apend.bits = bits;
    d->apend.d_out = d_out;
    d->apend.out_len = out_len;
    d->apend.st = st;
    d->apend.ro = ro;
    return HH_OK;
}

extern "C" int hh_decode_device_async(hh_decoder *d, const void *d_data, uint64_t bits, void *d_out,
                                      uint64_t cap, uint64_t *out_len, void *hip_stream) {
    if (!out_len || !decode_args_ok(d, d_data, bits, d_out, cap)) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    *out_len = 0;
    const bool fixed = fixed_code_path(d);
    if (bits == 0 || !(fixed || fsm_path_ok(d))) {
        // the other paths decode synchronously (the pending decode first);
        // whatever they return is reported by hh_decode_wait
        async_check(d);
        async_note(d, hh_decode_device(d, d_data, bits, d_out, cap, out_len, hip_stream));
        return HH_OK;
    }
    const int rc = async_enqueue(d, fixed, d_data, bits, 0, 0, 0, d_out, cap, out_len, nullptr, (hipStream_t)hip_stream);
    // intentional, pinned by the contract tests: a launch-time capacity failure is hh_decode_wait's to report
    return rc == HH_ERR_CAPACITY ? HH_OK : rc;
}

extern "C" int hh_decode_wait(hh_decoder *d) {
    if (!d) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);
    const int rc = d->async_rc;
    d->async_rc = HH_OK;
    return rc;
}

// ---------------------------------------------------------------------------
// The batched decode (hh_batch.hip): the arguments are checked here, before
// anything is launched or written.
// ---------------------------------------------------------------------------
extern "C" int hh_decode_batch_device(hh_decoder *d, const void *d_data, uint64_t data_bytes,
                                      const hh_batch_item *items, uint64_t n, void *d_out, uint64_t out_bytes,
                                      uint64_t *out_len, int32_t *status, void *hip_stream) {
    if (!d) return HH_ERR_ARG;
    if (n == 0) return HH_OK;
    if (!items || !out_len || !d_data || !d_out || !d->have_tree) return HH_ERR_ARG;
    if (((uintptr_t)d_data & 3u) != 0) return HH_ERR_ARG;   // word loads
    for (uint64_t i = 0; i < n; i++) {
        const hh_batch_item &s = items[i];
        if (s.data_off % 4u) return HH_ERR_ARG;
        if (s.bits) {
            const uint64_t nb = s.bits / 8u + (s.bits % 8u != 0) + HH_PAYLOAD_PAD;   // (bits / 8 <= 2^61: no overflow)
            if (s.data_off > data_bytes || nb > data_bytes - s.data_off) return HH_ERR_ARG;
        }
        if (s.out_off > out_bytes || s.cap > out_bytes - s.out_off) return HH_ERR_ARG;
    }
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);                     // (an asynchronous decode before it: its status is kept for hh_decode_wait)
    memset(&d->stats, 0, sizeof(d->stats));
    float ms = 0;
    uint64_t lanes = 0;
    const int rc = batch_decode(&d->batch, &d->fsm, d->ev, d_data, items, n, d_out, out_len, status,
                                (hipStream_t)hip_stream, &ms, &lanes);
    if (rc == HH_ERR_DEVICE || rc == HH_ERR_NOMEM || rc == HH_ERR_UNSUPPORTED) return rc;   // (nothing decoded)
    d->stats.ms_total = ms;
    d->stats.lanes = lanes;
    for (uint64_t i = 0; i < n; i++) d->stats.out_len += out_len[i];
    d->stats.state_machine = 3;
    return rc;
}

// The batch from a device list: only what the host can know is checked here;
// the items are checked by the kernel that reads them (hh_batch_plan.hip).
// Nothing here waits for the device, and a pending asynchronous decode stays
// pending (it shares no workspace with the batch).
extern "C" int hh_decode_batch_device_items(hh_decoder *d, const void *d_data, uint64_t data_bytes,
                                            const hh_batch_item *d_items, uint64_t n, void *d_out,
                                            uint64_t out_bytes, uint64_t *d_out_len, int32_t *d_status,
                                            hh_batch_summary *d_summary, void *hip_stream) {
    if (!d) return HH_ERR_ARG;
    if (n == 0) {
        if (!d_summary) return HH_OK;
        HIP_OK(hipSetDevice(d->device));
        return batch_summary_clear(d_summary, (hipStream_t)hip_stream);
    }
    if (!d_items || !d_out_len || !d_status || !d_data || !d_out || !d->have_tree) return HH_ERR_ARG;
    if (((uintptr_t)d_data & 3u) != 0) return HH_ERR_ARG;   // word loads
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    HIP_OK(hipSetDevice(d->device));
    const int rc = batch_decode_items(&d->batch, &d->fsm, d_data, data_bytes, d_items, n, d_out, out_bytes, d_out_len,
                                      d_status, d_summary, (hipStream_t)hip_stream);
    if (rc != HH_OK) return rc;
    memset(&d->stats, 0, sizeof(d->stats));                // (the host knows no lengths)
    d->stats.state_machine = 3;
    return HH_OK;
}

// Range reads over a blocked buffer: the host sees neither the reads nor the
// index, so it checks the pointers, the tree and the piece budget (before any
// allocation); the rest is the plan's kernels' (hh_batch_read.hip).
extern "C" int hh_decode_blocks_read(hh_decoder *d, const void *d_data, uint64_t data_bytes,
                                     const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms,
                                     const hh_block_read *d_reads, uint64_t m, void *d_out, uint64_t out_bytes,
                                     uint64_t *d_read_len, int32_t *d_status, hh_batch_summary *d_summary,
                                     void *hip_stream) {
    if (!d) return HH_ERR_ARG;
    if (m == 0) {
        if (!d_summary) return HH_OK;
        HIP_OK(hipSetDevice(d->device));
        return batch_summary_clear(d_summary, (hipStream_t)hip_stream);
    }
    if (!d_reads || !d_read_len || !d_status || !d_data || !d_out || !d->have_tree) return HH_ERR_ARG;
    if ((!d_index && n_syms > 0) || block_syms == 0) return HH_ERR_ARG;
    if (((uintptr_t)d_data & 3u) != 0) return HH_ERR_ARG;   // word loads
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    uint64_t P = 0;
    if (!hbr_budget(out_bytes, block_syms, m, &P)) return HH_ERR_UNSUPPORTED;
    HIP_OK(hipSetDevice(d->device));
    const int rc = batch_decode_read(&d->batch, &d->fsm, d_data, data_bytes, d_index, n_syms, block_syms, d_reads, m,
                                     (uint32_t)P, d_out, out_bytes, d_read_len, d_status, d_summary,
                                     (hipStream_t)hip_stream);
    if (rc != HH_OK) return rc;
    memset(&d->stats, 0, sizeof(d->stats));                // (the host knows no lengths)
    d->stats.state_machine = 3;
    return HH_OK;
}

// Gathered range reads: hh_decode_blocks_read's checks, and the blocks must
// number below 2^32 - 1 (a few words per block are kept; before any allocation).
extern "C" int hh_decode_blocks_gather(hh_decoder *d, const void *d_data, uint64_t data_bytes,
                                       const hh_batch_item *d_index, uint64_t n_syms, uint64_t block_syms,
                                       const hh_block_read *d_reads, uint64_t m, void *d_out, uint64_t out_bytes,
                                       uint64_t *d_read_len, int32_t *d_status, hh_batch_summary *d_summary,
                                       void *hip_stream) {
    if (!d) return HH_ERR_ARG;
    if (m == 0) {
        if (!d_summary) return HH_OK;
        HIP_OK(hipSetDevice(d->device));
        return batch_summary_clear(d_summary, (hipStream_t)hip_stream);
    }
    if (!d_reads || !d_read_len || !d_status || !d_data || !d_out || !d->have_tree) return HH_ERR_ARG;
    if ((!d_index && n_syms > 0) || block_syms == 0) return HH_ERR_ARG;
    if (((uintptr_t)d_data & 3u) != 0) return HH_ERR_ARG;   // word loads
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    uint64_t P = 0, nb = 0;
    if (!hbr_budget(out_bytes, block_syms, m, &P) || !hbg_blocks(n_syms, block_syms, &nb)) return HH_ERR_UNSUPPORTED;
    HIP_OK(hipSetDevice(d->device));
    const int rc = batch_decode_gather(&d->batch, &d->fsm, d_data, data_bytes, d_index, n_syms, block_syms, d_reads, m,
                                       (uint32_t)P, (uint32_t)nb, d_out, out_bytes, d_read_len, d_status, d_summary,
                                       (hipStream_t)hip_stream);
    if (rc != HH_OK) return rc;
    memset(&d->stats, 0, sizeof(d->stats));                // (the host knows no lengths)
    d->stats.state_machine = 3;
    return HH_OK;
}

// The record take: the host sees neither the ids nor the index; the rest is
// the plan's kernels' (hh_batch_take.hip).
extern "C" int hh_decode_batch_take(hh_decoder *d, const void *d_data, uint64_t data_bytes,
                                    const hh_batch_item *d_index, uint64_t nrec, const uint64_t *d_ids, uint64_t m,
                                    void *d_out, uint64_t out_bytes, uint64_t *d_out_offs, int32_t *d_status,
                                    hh_batch_summary *d_summary, void *hip_stream) {
    if (!d) return HH_ERR_ARG;
    if (!d_ids && m != nrec) return HH_ERR_ARG;
    if (m == 0) {
        if (!d_summary) return HH_OK;
        HIP_OK(hipSetDevice(d->device));
        return batch_summary_clear(d_summary, (hipStream_t)hip_stream);
    }
    if (!d_out_offs || !d_status || !d_data || !d_out || (!d_index && nrec > 0) || !d->have_tree) return HH_ERR_ARG;
    if (((uintptr_t)d_data & 3u) != 0 || ((uintptr_t)d_out_offs & 7u) != 0) return HH_ERR_ARG;   // word, 64-bit accesses
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    HIP_OK(hipSetDevice(d->device));
    const int rc = batch_decode_take(&d->batch, &d->fsm, d_data, data_bytes, d_index, nrec, d_ids, m, d_out, out_bytes,
                                     d_out_offs, d_status, d_summary, (hipStream_t)hip_stream);
    if (rc != HH_OK) return rc;
    memset(&d->stats, 0, sizeof(d->stats));                // (the host knows no lengths)
    d->stats.state_machine = 3;
    return HH_OK;
}

extern "C" int hh_decode_take_round_tiles(const hh_decoder *d, uint32_t *tiles) {
    if (!d || !tiles || !d->have_tree) return HH_ERR_ARG;
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    uint32_t lds = 0;
    return batch_take_waves(&d->batch, &d->fsm, tiles, &lds);
}

extern "C" int hh_decode_batch_round_tiles(const hh_decoder *d, uint32_t *tiles) {
    if (!d || !tiles || !d->have_tree) return HH_ERR_ARG;
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    *tiles = d->batch.W;
    return HH_OK;
}

extern "C" int hh_decoder_tile_bits(const hh_decoder *d, uint64_t *tile_bits) {
    if (!d || !tile_bits || !d->have_tree) return HH_ERR_ARG;
    *tile_bits = (uint64_t)HH_NR * d->S;
    return HH_OK;
}

// A segment's results before its decode: nothing written, the chain leaves
// in the state it entered.
static void range_out_init(hh_range_out *ro, const hh_range *rg) {
    memset(ro, 0, sizeof(*ro));
    ro->leave_state = ro->entry_state = rg->in_state;
    ro->entry_exact = rg->prologue == 0;
}

extern "C" int hh_decode_device_range(hh_decoder *d, const void *d_data, const hh_range *rg,
                                      void *d_out, uint64_t cap, hh_range_out *ro,
                                      void *hip_stream) {
    if (!rg || !ro || !decode_args_ok(d, d_data, rg->bits_avail, d_out, cap)) return HH_ERR_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);
    memset(&d->stats, 0, sizeof(d->stats));
    range_out_init(ro, rg);
    // no tiles (a shard with none of its own when there are fewer tiles than
    // ranks): that is the result
    if (rg->bits_avail == 0 || rg->ntiles == 0) return HH_OK;
    if (fsm_path_ok(d)) {
        // states are state-machine states (0: the root, the stream start)
        if (rg->in_state >= d->fsm.ns) return HH_ERR_ARG;
        float ms[4] = {0, 0, 0, 0};
        const int rc = fsm_decode(&d->fsm, &d->fsm_ws, d->ev, d_data, rg->bits_avail, rg->ntiles, rg->in_state,
                                  rg->prologue, d_out, cap, st, &ro->out_len, &ro->leave_state, &ro->entry_state, ms);
        fsm_stats(d, rg->bits_avail, ro->out_len, ms, d->fsm_ws.last_one);
        if (rc == HH_NOSYNC) return HH_ERR_UNSUPPORTED;   // (decode such a code whole)
        // the state leaving a segment does not depend on how it was entered
        // once the chain from its entry has met an entry-independent one
        // (a head's).  The count pass proves that meeting only through a
        // tile's lane-63 walk into its successor (a chain that does not meet
        // there fails the decode), so only a segment of two or more count
        // tiles has a leave state proven independent of its entry (the count
        // pass's tiles: fsm.cm emission tiles each); a one-tile segment's is
        // valid only when its entry is.  The entry after a prologue is
        // checked against the predecessor's leave state by the caller.
        ro->const_seen = rg->ntiles > (uint64_t)d->fsm.cm;
        return rc;
    }
    // segments need the fast path (tile tables, entry states); a tree it
    // does not support is decoded whole, unsharded
    if (!fast_path_ok(d) || hh_state_d(rg->in_state) >= HH_KM) return HH_ERR_UNSUPPORTED;
    uint32_t cp = 0;
    const int rc = decode_fast(d, d_data, rg->bits_avail, rg->ntiles, rg->in_state, rg->prologue,
                               d_out, cap, st, &ro->out_len, &ro->leave_state, &cp,
                               &ro->const_seen, &ro->entry_state);
    ro->entry_exact = rg->prologue == 0 || cp != 0;
    return rc == HH_NOSYNC ? HH_ERR_UNSUPPORTED : rc;
}

// The asynchronous form (multi-GPU shards: a stream of segment decodes with
// no host wait between them).  ro is filled when the decode is checked: by
// the next asynchronous decode on this decoder or by hh_decode_wait.
extern "C" int hh_decode_device_range_async(hh_decoder *d, const void *d_data, const hh_range *rg,
                                            void *d_out, uint64_t cap, hh_range_out *ro,
                                            void *hip_stream) {
    if (!rg || !ro || !decode_args_ok(d, d_data, rg->bits_avail, d_out, cap)) return HH_ERR_ARG;
    if (!fsm_path_ok(d) || rg->bits_avail == 0 || rg->ntiles == 0) {
        // (other paths, and empty segments: synchronously, as hh_decode_device_range)
        async_check(d);
        const int rc = hh_decode_device_range(d, d_data, rg, d_out, cap, ro, hip_stream);
        async_note(d, rc);
        // intentional, pinned by the contract tests: the synchronous decode's capacity failure is hh_decode_wait's to report
        return rc == HH_ERR_CAPACITY ? HH_OK : rc;
    }
    if (rg->in_state >= d->fsm.ns) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    range_out_init(ro, rg);
    // (known at launch: see hh_decode_device_range)
    ro->const_seen = rg->ntiles > (uint64_t)d->fsm.cm;
    // intentional, pinned by the contract tests: a launch-time failure, HH_ERR_CAPACITY too, is returned as it is
    return async_enqueue(d, false, d_data, rg->bits_avail, rg->ntiles, rg->in_state, rg->prologue, d_out, cap,
                         &ro->out_len, ro, (hipStream_t)hip_stream);
}

// Diagnostic: the state-machine count pass's arrays of the last decode of
// `ntiles` tiles (records, corrections, tile sums, leaving states).
extern "C" int hh_debug_fsm(hh_decoder *d, uint64_t ntiles, uint32_t *rec, uint32_t *fx, int32_t *tsum,
                            uint32_t *xs) {
    if (!d) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    return fsm_debug_arrays(&d->fsm_ws, ntiles, rec, fx, tsum, xs);
}

// Diagnostic: the geometry hh_decoder_set_tree chose for the batched decode:
// region bits S, emission step K, remainder step r, count step bits cb, the
// batch's head G, its waves per round W, the states ns, k_batch's LDS bytes.
// Host fields only: no device call.
extern "C" int hh_debug_geometry(hh_decoder *d, uint32_t out[8]) {
    if (!d || !out || !d->have_tree) return HH_ERR_ARG;
    if (!d->fsm.ok || !d->batch.ok) return HH_ERR_UNSUPPORTED;
    out[0] = d->fsm.S;
    out[1] = d->fsm.K;
    out[2] = d->fsm.r;
    out[3] = d->fsm.cb;
    out[4] = d->batch.G;
    out[5] = d->batch.W;
    out[6] = d->fsm.ns;
    out[7] = d->batch.lds;
    return HH_OK;
}
