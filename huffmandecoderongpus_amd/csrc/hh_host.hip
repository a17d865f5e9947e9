// hh_host.hip -- decodes from and to host memory (hh_decode_host): staged
// copies through pinned chunk buffers, and the pipelined form over the
// caller's page-locked buffers.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

#include "hh_algo.h"
#include "hh_dec.h"
#include "hh_internal.h"
#include "hiphuff.h"

// evaluate() scope (decodeUtil.c:41-43 times the whole decoder call): host
// payload in, host symbols out.  Copies go through two pinned chunk buffers
// the decoder keeps (HH_HOST_CHUNK each): the CPU copy of one chunk into (or
// out of) pinned memory overlaps the DMA of the other, both ways.  Device
// buffers are kept too: no allocation after the first call of a size.
#define HH_HOST_CHUNK ((size_t)64 << 20)
#define HH_HOST_THREADS 8                  // CPU copies into / out of pinned memory

// The CPU side of a chunk: a single core copies ~10 GB/s, below PCIe's
// rate, so the chunk is split over a few threads.
static void par_memcpy(uint8_t *dst, const uint8_t *src, size_t len) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::min<size_t>(hw ? std::min<unsigned>(hw, HH_HOST_THREADS) : 1, len >> 20);
    if (nt <= 1) {
        memcpy(dst, src, len);
        return;
    }
    std::thread th[HH_HOST_THREADS];
    const size_t part = (len / nt + 4095) & ~(size_t)4095;
    for (size_t i = 1; i < nt; i++) {
        const size_t o = i * part;
        if (o >= len) continue;
        try {
            th[i] = std::thread(memcpy, dst + o, src + o, std::min(part, len - o));
        } catch (...) {   // (no thread to be had: this part on the calling thread)
            memcpy(dst + o, src + o, std::min(part, len - o));
        }
    }
    memcpy(dst, src, std::min(part, len));
    for (size_t i = 1; i < nt; i++)
        if (th[i].joinable()) th[i].join();
}

static int host_pipe(hh_decoder *d, uint8_t *host, uint8_t *dev, size_t n, bool h2d) {
    if (!n) return HH_OK;
    const size_t nch = (n + HH_HOST_CHUNK - 1) / HH_HOST_CHUNK;
    for (size_t i = 0; i < nch + 1; i++) {
        // DMA chunk i (h2d: after the CPU has staged it; d2h: into its buffer)
        if (i < nch) {
            const size_t off = i * HH_HOST_CHUNK, len = n - off < HH_HOST_CHUNK ? n - off : HH_HOST_CHUNK;
            uint8_t *pin = d->h_stage + (i & 1) * HH_HOST_CHUNK;
            if (i >= 2) HIP_OK(hipEventSynchronize(d->h_ev[i & 1]));   // buffer free again
            if (h2d) {
                par_memcpy(pin, host + off, len);
                HIP_OK(hipMemcpyAsync(dev + off, pin, len, hipMemcpyHostToDevice, d->stream));
            } else {
                HIP_OK(hipMemcpyAsync(pin, dev + off, len, hipMemcpyDeviceToHost, d->stream));
            }
            HIP_OK(hipEventRecord(d->h_ev[i & 1], d->stream));
        }
        // d2h: the CPU drains chunk i-1 while chunk i is in flight
        if (!h2d && i >= 1) {
            const size_t k = i - 1, off = k * HH_HOST_CHUNK;
            const size_t len = n - off < HH_HOST_CHUNK ? n - off : HH_HOST_CHUNK;
            HIP_OK(hipEventSynchronize(d->h_ev[k & 1]));
            par_memcpy(host + off, d->h_stage + (k & 1) * HH_HOST_CHUNK, len);
        }
    }
    return HH_OK;
}

// The evaluate() scope, pipelined (state-machine path): the caller's buffers
// are page-locked for the call (hipHostRegister) so that the DMA engines read
// and write them directly; the payload goes up in chunks of whole tiles on
// one copy stream, chunk k is decoded as a segment as soon as it has landed
// (entered in the state chunk k-1 left), and its symbols go down on a second
// copy stream while later chunks are still uploading and decoding.
#define HH_PIPE_CHUNK ((uint64_t)128 << 20)          // payload bytes per chunk

static uint64_t pipe_chunk() {
    const char *e = getenv("HH_PIPE_CHUNK_KB");        // (tests: force many chunks)
    const uint64_t v = e ? strtoull(e, nullptr, 10) << 10 : 0;
    return v ? v : HH_PIPE_CHUNK;
}

// HH_FLAG_KEEP_HOST_PINNED: buffer k (0 payload, 1 output) page-locked
// from p for at least n bytes, the registration kept for later calls.
// Registrations are whole pages and may not overlap: a buffer whose pages
// lie inside the other buffer's registration is recorded as covered by it
// (pin_own 0), one that overlaps it partly gets a registration of the union
// of both (the other then covered by it); when a registration goes, the
// buffer it covered is pinned again.
static bool pin_inside(const hh_decoder *d, int k, uintptr_t a, uintptr_t b) {
    return d->pin_p[k] && d->pin_own[k] && a >= d->pin_ra[k] && b <= d->pin_rb[k];
}
static void pin_drop(hh_decoder *d, int k) {
    if (d->pin_p[k] && d->pin_own[k]) (void)hipHostUnregister((void *)d->pin_ra[k]);
    d->pin_p[k] = nullptr;
    d->pin_n[k] = 0;
    d->pin_own[k] = 0;
    d->pin_ra[k] = d->pin_rb[k] = 0;
}
static int pin_host(hh_decoder *d, int k, const void *p, size_t n) {
    uintptr_t a = (uintptr_t)p & ~(uintptr_t)4095, b = ((uintptr_t)p + n + 4095) & ~(uintptr_t)4095;
    if (d->pin_p[k] == p && d->pin_n[k] >= n && (d->pin_own[k] || pin_inside(d, k ^ 1, a, b))) return HH_OK;
    const int o = k ^ 1;
    const void *op = d->pin_p[o];
    const size_t on = d->pin_n[o];
    bool repin = op && !d->pin_own[o];               // (o relied on k's registration)
    pin_drop(d, k);
    if (pin_inside(d, o, a, b)) {                     // (within the other buffer's pages)
        d->pin_p[k] = p;
        d->pin_n[k] = n;
        return HH_OK;
    }
    if (op && d->pin_own[o] && a < d->pin_rb[o] && d->pin_ra[o] < b) {
        // a partial overlap: one registration of both
        a = std::min(a, d->pin_ra[o]);
        b = std::max(b, d->pin_rb[o]);
        pin_drop(d, o);
        repin = true;
    }
    if (hipHostRegister((void *)a, b - a, hipHostRegisterDefault) != hipSuccess) return HH_ERR_UNSUPPORTED;
    d->pin_p[k] = p;
    d->pin_n[k] = n;
    d->pin_own[k] = 1;
    d->pin_ra[k] = a;
    d->pin_rb[k] = b;
    return repin ? pin_host(d, o, op, on) : HH_OK;
}

extern "C" int hh_decoder_release_host(hh_decoder *d) {
    if (!d) return HH_ERR_ARG;
    for (int k = 0; k < 2; k++) pin_drop(d, k);
    return HH_OK;
}

static int host_pipeline(hh_decoder *d, const uint8_t *data, uint64_t bits, uint8_t *out, uint64_t cap,
                         uint64_t *out_len) {
    const uint64_t nb = (bits + 7) / 8;
    const uint64_t tbb = (uint64_t)HH_NR * d->S / 8;                 // bytes per tile
    const uint64_t ch = pipe_chunk() > tbb ? pipe_chunk() / tbb * tbb : tbb;
    const uint64_t nch = (nb + ch - 1) / ch;
    if (!d->h2d) {
        HIP_OK(hipStreamCreateWithFlags(&d->h2d, hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&d->d2h, hipStreamNonBlocking));
    }
    if (nch > d->npipe_ev) {
        for (uint32_t i = 0; i < d->npipe_ev; i++) (void)hipEventDestroy(d->pipe_ev[i]);
        free(d->pipe_ev);
        d->npipe_ev = 0;
        d->pipe_ev = (hipEvent_t *)calloc(nch, sizeof(hipEvent_t));
        if (!d->pipe_ev) return HH_ERR_NOMEM;
        for (uint64_t i = 0; i < nch; i++) {
            HIP_OK(hipEventCreateWithFlags(&d->pipe_ev[i], hipEventDisableTiming));
            d->npipe_ev = (uint32_t)(i + 1);
        }
    }
    const bool keep = (d->cfg.flags & HH_FLAG_KEEP_HOST_PINNED) != 0;
    if (keep) {
        // the buffers stay registered across calls: (re)register only a new
        // pointer or a longer length
        if (pin_host(d, 0, data, nb) != HH_OK) return HH_ERR_UNSUPPORTED;
        if (cap && pin_host(d, 1, out, cap) != HH_OK) return HH_ERR_UNSUPPORTED;
    } else {
        if (hipHostRegister((void *)data, nb, hipHostRegisterDefault) != hipSuccess) return HH_ERR_UNSUPPORTED;
        if (cap && hipHostRegister(out, cap, hipHostRegisterDefault) != hipSuccess) {
            (void)hipHostUnregister((void *)data);
            return HH_ERR_UNSUPPORTED;
        }
    }
    int rc = HH_OK;
    uint8_t *din = (uint8_t *)d->d_in, *dout = (uint8_t *)d->d_out;
    if (hipMemsetAsync(din + nb, 0, HH_PAYLOAD_PAD, d->h2d) != hipSuccess) rc = HH_ERR_DEVICE;
    for (uint64_t k = 0; k < nch && !rc; k++) {
        const uint64_t o = k * ch, len = nb - o < ch ? nb - o : ch;
        if (hipMemcpyAsync(din + o, data + o, len, hipMemcpyHostToDevice, d->h2d) != hipSuccess ||
            hipEventRecord(d->pipe_ev[k], d->h2d) != hipSuccess)
            rc = HH_ERR_DEVICE;
    }
    uint64_t total = 0;
    uint32_t state = 0;
    bool over = false;
    float ms_all[4] = {0, 0, 0, 0};
    for (uint64_t k = 0; k < nch && !rc; k++) {
        const uint64_t b0 = k * ch * 8;
        const uint64_t ntiles = (k + 1 < nch ? ch * 8 : bits - b0 + d->S * HH_NR - 1) / (d->S * HH_NR);
        // readable bits: the chunk and the first tile of the next (the stream
        // end lies beyond a chunk's tiles, except in the last one)
        const uint64_t avail = bits - b0 < (ch + tbb) * 8 ? bits - b0 : (ch + tbb) * 8;
        if (hipStreamWaitEvent(d->stream, d->pipe_ev[k], 0) != hipSuccess) { rc = HH_ERR_DEVICE; break; }
        // (the first tile of the next chunk may not have landed yet: the
        // kernels read it only for chains that this segment does not use)
        uint64_t n = 0;
        uint32_t leave = 0, en = 0;
        float ms[4] = {0, 0, 0, 0};
        // (past a capacity failure the later chunks are only counted -- no
        // room is left, nothing is written -- so that out_len is the stream's
        // total, as hh_decode_device reports it)
        const uint64_t room = over || total >= cap ? 0 : cap - total;
        rc = fsm_decode(&d->fsm, &d->fsm_ws, d->ev, din + k * ch, avail, ntiles, state, 0,
                        room ? dout + total : dout, room, d->stream, &n, &leave, &en, ms);
        if (rc == HH_ERR_CAPACITY) {
            over = true;
            rc = HH_OK;
        }
        if (rc) break;
        for (int i = 0; i < 4; i++) ms_all[i] += ms[i];
        if (!over && n && hipMemcpyAsync(out + total, dout + total, n, hipMemcpyDeviceToHost, d->d2h) != hipSuccess) {
            rc = HH_ERR_DEVICE;
            break;
        }
        total += n;
        state = leave;
    }
    if (over && !rc) rc = HH_ERR_CAPACITY;
    if (hipStreamSynchronize(d->d2h) != hipSuccess || hipStreamSynchronize(d->h2d) != hipSuccess) rc = rc ? rc : HH_ERR_DEVICE;
    if (!keep) {
        (void)hipHostUnregister((void *)data);
        if (cap) (void)hipHostUnregister(out);
    }
    fsm_stats(d, bits, total, ms_all, d->fsm_ws.last_one);
    *out_len = total;
    return rc == HH_NOSYNC ? HH_ERR_UNSUPPORTED : rc;   // (no resync: the serial path decodes it whole)
}

extern "C" int hh_decode_host(hh_decoder *d, const uint8_t *data, uint64_t bits, uint8_t *out,
                              uint64_t cap, uint64_t *out_len) {
    if (!d || !out_len || (!data && bits) || (!out && cap)) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    async_check(d);
    *out_len = 0;
    const uint64_t nb = (bits + 7) / 8;
    const uint64_t ocap = cap ? cap : 1;
    int rc = ensure_dev(&d->d_in, &d->d_in_size, nb + HH_PAYLOAD_PAD);
    if (!rc) rc = ensure_dev(&d->d_out, &d->d_out_size, ocap);
    if (rc) return rc;
    if (!d->h_stage) {
        if (hipHostMalloc((void **)&d->h_stage, 2 * HH_HOST_CHUNK, hipHostMallocDefault) != hipSuccess) {
            d->h_stage = nullptr;
            return HH_ERR_NOMEM;
        }
        if (hipEventCreateWithFlags(&d->h_ev[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&d->h_ev[1], hipEventDisableTiming) != hipSuccess)
            return HH_ERR_DEVICE;
    }
    if (fsm_path_ok(d) && nb > pipe_chunk() && !getenv("HH_HOST_SERIAL")) {
        rc = host_pipeline(d, data, bits, out, cap, out_len);
        if (rc != HH_ERR_UNSUPPORTED) return rc;   // (unsupported: registration refused -> staged copies)
        rc = HH_OK;
    }
    HIP_OK(hipMemsetAsync((uint8_t *)d->d_in + nb, 0, HH_PAYLOAD_PAD, d->stream));
    rc = host_pipe(d, (uint8_t *)data, (uint8_t *)d->d_in, nb, true);
    if (!rc) rc = hh_decode_device(d, d->d_in, bits, d->d_out, cap, out_len, d->stream);
    if (!rc) rc = host_pipe(d, out, (uint8_t *)d->d_out, *out_len, false);
    if (!rc) HIP_OK(hipStreamSynchronize(d->stream));
    return rc;
}
