// Byte histogram on the device: the counting pass in front of the encoder
// (hh_compress_device, csrc/hh_encode.hip).  Reads every input byte once;
// kernels and LDS layout in hh_hist_kern.h.  Two launches on the caller's
// stream (k_hist, k_hist_sum), then the host reads 2 KiB.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hiphuff.h"
#include "hh_enc.h"
#include "hh_hist_kern.h"

// LDS copies per workgroup and workgroups per CU: the best of
// tools/ubench/ub_hist.hip's sweep on 256 MiB of tiled bible.txt (1..32
// copies x 2..16 workgroups per CU; DESIGN.md "Compression": 1 copy 1.40
// TB/s, 8 copies 2.90, 32 copies 3.71 at 2 per CU; more workgroups per CU
// are slower at every copy count).  32 copies are 32.1 KiB of LDS per
// workgroup.
#ifndef HIST_COPIES
#define HIST_COPIES 32
#endif
#ifndef HIST_WG_PER_CU
#define HIST_WG_PER_CU 2
#endif

// A workgroup's LDS counters are u32 and are flushed once, at its end, so
// its whole share of the input must stay below 2^32 bytes.  The grid-stride
// loop gives a workgroup at most ceil(nvec / (grid * HIST_TB)) * HIST_TB
// vectors of 16 B (<= n / grid + 16 * HIST_TB bytes) plus 30 single bytes;
// with grid >= ceil(n / HIST_WG_MAX_BYTES) that is at most
// 2^31 + 4096 + 30 < 2^32 on any device, however few CUs it has.
#define HIST_WG_MAX_BYTES (1ull << 31)

extern "C" int hh_histogram_device(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t counts[256],
                                   void *hip_stream) {
    if (!enc || !counts || (!d_syms && n)) return HH_ERR_ARG;
    memset(counts, 0, 256 * sizeof(uint64_t));
    if (n == 0) return HH_OK;
    // (the encoder's limit: its launch of one workgroup of 256 per 4096 symbols)
    if ((n + 4095) / 4096 * 256 > 0xffffffffull) return HH_ERR_UNSUPPORTED;
    if (hipSetDevice(enc->device) != hipSuccess) return HH_ERR_DEVICE;
    if (!enc->cus) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, enc->device) != hipSuccess || cus <= 0)
            return HH_ERR_DEVICE;
        enc->cus = cus;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // the persistent grid; never more workgroups than the input has vectors
    // for (small inputs), never fewer than the overflow bound asks
    uint64_t grid = (uint64_t)enc->cus * HIST_WG_PER_CU;
    const uint64_t useful = (n / 16 + HIST_TB - 1) / HIST_TB;
    if (grid > useful) grid = useful ? useful : 1;
    const uint64_t floor_wgs = (n + HIST_WG_MAX_BYTES - 1) / HIST_WG_MAX_BYTES;
    if (grid < floor_wgs) grid = floor_wgs;
    const size_t o_cnt = (size_t)grid * 256 * sizeof(uint32_t), need = o_cnt + 256 * sizeof(uint64_t);
    if (enc->hist_size < need) {
        // (the previous call on this encoder has returned: nothing in flight)
        if (enc->hist_ws) (void)hipFree(enc->hist_ws);
        enc->hist_ws = nullptr;
        enc->hist_size = 0;
        if (hipMalloc(&enc->hist_ws, need) != hipSuccess) return HH_ERR_NOMEM;
        enc->hist_size = need;
    }
    uint32_t *d_slab = (uint32_t *)enc->hist_ws;
    uint64_t *d_cnt = (uint64_t *)(enc->hist_ws + o_cnt);
    hipLaunchKernelGGL(k_hist<HIST_COPIES>, dim3((unsigned)grid), dim3(HIST_TB), 0, st, (const uint8_t *)d_syms, n,
                       d_slab);
    if (hipGetLastError() != hipSuccess) return HH_ERR_DEVICE;
    hipLaunchKernelGGL(k_hist_sum, dim3(HIST_SUM_WGS), dim3(HIST_SUM_TB), 0, st, d_slab, (uint32_t)grid, d_cnt);
    if (hipGetLastError() != hipSuccess) return HH_ERR_DEVICE;
    if (hipMemcpyAsync(counts, d_cnt, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return HH_ERR_DEVICE;
    if (hipStreamSynchronize(st) != hipSuccess) return HH_ERR_DEVICE;
    return HH_OK;
}
