// hh_exact.hip -- the three exact paths beside the chain decodes: k_fixed (a
// complete fixed-length code), the segment path (any code of at most 32 bits,
// whether or not it resynchronises) and the reference-shaped stage kernels
// (k_st_*), which mirror the six .cl kernels one by one for intermediate-array
// parity, with the stage API and the pipeline that drives them.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "hh_algo.h"
#include "hh_dec.h"
#include "hh_internal.h"
#include "hiphuff.h"

// ---------------------------------------------------------------------------
// k_fixed: a complete fixed-length code (2^L symbols, every code L <= 8
// bits) needs no chain: symbol i is the L bits at i * L.  One thread per 16
// symbols, a 16-B store each; the stream's last code, if the end cuts it,
// takes the reference's tail rule (the node its bits reach,
// decodeallbits.cl:20-31).  sym[w] is the symbol of the L-bit window w
// (stream bit p in bit 0).
// ---------------------------------------------------------------------------
#ifndef HH_FIXED_NT
#define HH_FIXED_NT 1         // k_fixed's 16-B output stores nontemporal (E.coli 1 GiB 1.063 -> 1.048 ms)
#endif
__device__ __forceinline__ void fixed_store16(uint8_t *p, u32x4 v) {
    if (HH_FIXED_NT) __builtin_nontemporal_store(v, (u32x4 *)p);
    else *(u32x4 *)p = v;
}
__global__ __launch_bounds__(256) void k_fixed(const uint32_t *__restrict__ gdata, uint64_t bits, uint32_t L,
                                               const uint8_t *__restrict__ fsym, DevTab tab,
                                               uint8_t *__restrict__ out, uint64_t nsym) {
    __shared__ uint8_t s_sym[256];
    __shared__ uint32_t s_b4[256];                      // L = 2: a byte's four symbols
    const bool a16 = ((uintptr_t)out & 15u) == 0;
    s_sym[threadIdx.x] = fsym[threadIdx.x];
    {
        const uint32_t b = threadIdx.x;
        s_b4[b] = fsym[b & 3u] | (uint32_t)fsym[(b >> 2) & 3u] << 8 | (uint32_t)fsym[(b >> 4) & 3u] << 16 |
                  (uint32_t)fsym[b >> 6] << 24;
    }
    __syncthreads();
    const uint64_t nfull = bits / L;                    // whole codes
    const uint32_t mask = (1u << L) - 1u;
    const uint64_t G = (uint64_t)gridDim.x * blockDim.x;
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (L == 2 && a16) {
        // (E.coli) four groups per pass, their words loaded together: one
        // word -> four byte lookups -> one 16-B store each
        for (; (g + 3 * G) * 16 + 16 <= nfull; g += 4 * G) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) w[u] = gdata[g + u * G];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++)
                fixed_store16(out + (g + u * G) * 16, (u32x4){s_b4[w[u] & 255u], s_b4[(w[u] >> 8) & 255u],
                                                              s_b4[(w[u] >> 16) & 255u], s_b4[w[u] >> 24]});
        }
    }
    for (; g * 16 < nsym; g += G) {
        const uint64_t i0 = g * 16, p0 = i0 * L;
        if (L == 2 && i0 + 16 <= nfull && a16) {       // (E.coli) one word, four byte lookups
            const uint32_t w = gdata[g];
            fixed_store16(out + i0, (u32x4){s_b4[w & 255u], s_b4[(w >> 8) & 255u], s_b4[(w >> 16) & 255u],
                                            s_b4[w >> 24]});
            continue;
        }
        uint64_t wi = p0 >> 5;
        uint64_t buf = ((uint64_t)gdata[wi + 1] << 32 | gdata[wi]) >> (p0 & 31);
        uint32_t have = 64 - (uint32_t)(p0 & 31);
        wi += 2;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            if (have < L) {                             // (L <= 8: one word tops it up)
                buf |= (uint64_t)gdata[wi++] << have;
                have += 32;
            }
            v[k >> 2] |= (uint32_t)s_sym[(uint32_t)buf & mask] << (8 * (k & 3));
            buf >>= L;
            have -= L;
        }
        if (i0 + 16 <= nfull && a16) {
            *(u32x4 *)(out + i0) = (u32x4){v[0], v[1], v[2], v[3]};
        } else {                                        // the stream's end (or an unaligned output)
            for (uint32_t k = 0; k < 16 && i0 + k < nsym; k++) {
                uint8_t b = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
                if (i0 + k == nfull) {                  // a code cut by the end: the tail rule
                    uint32_t node = 0;
                    for (uint64_t p = nfull * L; p < bits; p++) {
                        const uint32_t tn = tab.tree[node];
                        if (tn & HH_T_LEAF) break;
                        const uint32_t bit = (gdata[p >> 5] >> (p & 31)) & 1u;
                        node = bit ? (tn >> 15) & 0x7fffu : tn & 0x7fffu;
                    }
                    b = tab.tsym[node];
                }
                out[i0 + k] = b;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Segment path: exact and O(N) for any code of at most 32 bits, whether or
// not it resynchronises (the fast path's walks need it to).  The stream is
// cut into segments of `seglen` bits.  The chain through a segment is fixed
// by the offset o in [0, maxadv) of its first boundary past the segment
// start, so k_seg_func decodes every segment from every o (one lane each):
// the exit offset into the next segment and the symbols starting in the
// segment.  The host composes the maps from segment 0 (offset 0): entry
// offsets and output bases.  k_seg_emit re-decodes every segment from its
// true entry (one lane each) straight to HBM.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void seg_ctx(hh_ctx &c, const uint32_t *gdata, uint64_t seg0, uint64_t bits,
                                        uint32_t seglen, const uint32_t *s_l1m, const DevTab &tab,
                                        uint32_t maxadv) {
    c.w = gdata + seg0 / 32;                            // linear words of the segment:
    c.sw = 1;                                           // hh_idx(g) == g
    c.nls = 1;
    c.magic = 0;
    c.l1m = s_l1m;
    c.l1s = nullptr;
    c.l1 = nullptr;
    c.l2 = tab.l2;
    c.tree = tab.tree;
    c.tsym = tab.tsym;
    c.maxadv = maxadv;
    c.G = 0;
    const uint64_t rem = bits - seg0;
    const uint64_t lim = (uint64_t)seglen + 2 * maxadv;
    c.bt = (uint32_t)(rem < lim ? rem : lim);
}

__global__ __launch_bounds__(256) void k_seg_func(const uint32_t *__restrict__ gdata, uint64_t bits,
                                                  uint32_t seglen, uint32_t nseg, uint32_t no,
                                                  DevTab tab, uint32_t maxadv, uint32_t *exits,
                                                  uint32_t *counts) {
    __shared__ uint32_t s_l1m[HH_L1_SIZE];
    for (uint32_t i = threadIdx.x; i < HH_L1_SIZE; i += blockDim.x) s_l1m[i] = (uint32_t)(tab.l1[i] >> 32);
    __syncthreads();
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (uint64_t)nseg * no) return;
    const uint32_t sg = (uint32_t)(id / no), o = (uint32_t)(id % no);
    const uint64_t seg0 = (uint64_t)sg * seglen;
    hh_ctx c;
    seg_ctx(c, gdata, seg0, bits, seglen, s_l1m, tab, maxadv);
    const uint32_t end = c.bt < seglen ? c.bt : seglen;  // symbols starting before it count
    uint32_t n = 0, x = o;
    if (o < end) x = hh_region_count(&c, o, end, &n);
    exits[id] = x >= end ? x - end : 0u;                // offset into the next segment
    counts[id] = n;
}

__global__ __launch_bounds__(256) void k_seg_emit(const uint32_t *__restrict__ gdata, uint64_t bits,
                                                  uint32_t seglen, uint32_t nseg, DevTab tab,
                                                  uint32_t maxadv, const uint32_t *entry,
                                                  const uint32_t *exitv, const uint64_t *base,
                                                  uint8_t *__restrict__ out) {
    __shared__ uint32_t s_l1m[HH_L1_SIZE];
    __shared__ uint32_t s_l1s[HH_L1_SIZE];
    for (uint32_t i = threadIdx.x; i < HH_L1_SIZE; i += blockDim.x) {
        const uint64_t e = tab.l1[i];
        s_l1m[i] = (uint32_t)(e >> 32);
        s_l1s[i] = (uint32_t)e;
    }
    __syncthreads();
    const uint32_t sg = blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= nseg) return;
    const uint64_t seg0 = (uint64_t)sg * seglen;
    hh_ctx c;
    seg_ctx(c, gdata, seg0, bits, seglen, s_l1m, tab, maxadv);
    c.l1s = s_l1s;
    const uint32_t end = c.bt < seglen ? c.bt : seglen;
    const uint32_t e0 = entry[sg];
    // the run ends at the first boundary at or past the segment end (or bt)
    const uint32_t pe0 = end + exitv[sg], pe = pe0 < c.bt ? pe0 : c.bt;
    if (e0 >= end) return;
    uint8_t *ob = out + base[sg];
    hh_cur cu = hh_cur_at(&c, e0);
    uint64_t o = 0;
    uint32_t val, k;
    while (cu.p < pe) {
        hh_emit_step(&c, cu, pe, o, ~0ull, &val, &k);
        for (uint32_t i = 0; i < k; i++) ob[o + i] = (uint8_t)(val >> (8 * i));
        o += k;
    }
}

// ---------------------------------------------------------------------------
// Reference-shaped stage kernels (ReleaseCL/kernels/ *.cl, one each).
// ---------------------------------------------------------------------------
__global__ void k_st_init(int32_t *idx, int64_t bits) {
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x)
        idx[b] = -1;
}

// decodeallbits.cl:10-33: walk from every bit until a leaf or the end.
__global__ void k_st_decodeallbits(const uint8_t *__restrict__ data, int64_t bits, DevTab tab,
                                   uint8_t *__restrict__ bitdecode, int32_t *__restrict__ steps) {
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = b;
        uint32_t node = 0;
        for (;;) {
            uint32_t t = tab.tree[node];
            if ((t & HH_T_LEAF) || p >= bits) break;
            uint32_t bit = (data[p >> 3] >> (p & 7)) & 1u;
            node = bit ? (t >> 15) & 0x7fffu : t & 0x7fffu;
            p++;
        }
        bitdecode[b] = tab.tsym[node];
        steps[b] = (int32_t)(p - b);
    }
}

// makebigtable.cl:10-40 with the end-of-stream read made explicit: a span
// ending exactly at the end (b + s == bits) reads row step+1 in the serial
// form (pes.c:58) and always yields -1 there; here that case is -1 directly.
__global__ void k_st_makebigtable(int64_t bits, int32_t *steps, int32_t step) {
    const int32_t *cur = steps + (int64_t)step * bits;
    int32_t *nxt = steps + (int64_t)(step + 1) * bits;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x) {
        int32_t s = cur[b], v;
        if (s == -1 || b + s >= bits) {
            v = -1;
        } else {
            int32_t w = cur[b + s];
            v = (w == -1 || b + s + w > bits) ? -1 : s + w;
        }
        nxt[b] = v;
    }
}

// calcbitsindex.cl:5-22
__global__ void k_st_calcbitsindex(int64_t bits, int32_t *idx, const int32_t *steps, int32_t step,
                                   int32_t pw) {
    const int32_t *lv = steps + (int64_t)(step - 1) * bits;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x) {
        int32_t off = lv[b], cv = idx[b];
        if (off != -1 && cv != -1 && b + off < bits) idx[b + off] = cv + pw;
    }
}

// calcresult.cl:5-19
__global__ void k_st_calcresult(int64_t bits, const int32_t *idx, const uint8_t *bitdecode,
                                uint8_t *result, uint64_t cap) {
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x) {
        int32_t i = idx[b];
        if (i != -1 && (uint64_t)i < cap) result[i] = bitdecode[b];
    }
}

// findmax.cl:2-8 (max-reduction; the serial scan finds the same value)
__global__ void k_st_findmax(int64_t bits, const int32_t *idx, int32_t *maxv) {
    int32_t m = -1;
    for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; b < bits;
         b += (int64_t)gridDim.x * blockDim.x)
        m = idx[b] > m ? idx[b] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        int32_t y = __shfl_xor(m, o, 64);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(maxv, m);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static inline unsigned grid_for(int64_t n, unsigned bs) {
    int64_t g = (n + bs - 1) / bs;
    if (g > 65536) g = 65536;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// The segment path (above).  Memory: 8 bytes per (segment, offset) and 16
// per segment; the maps are composed on the host.
int segment_path(hh_decoder *d, const void *d_data, uint64_t bits, uint8_t *d_out, uint64_t cap,
                 uint64_t *out_len, hipStream_t st) {
    const uint32_t maxadv = d->ht->maxlen > HH_P ? (uint32_t)d->ht->maxlen : HH_P;
    const uint32_t no = (uint32_t)d->ht->maxlen;        // boundary offsets past a segment start
    const uint32_t seglen = 1u << 16;
    const uint64_t nseg64 = (bits + seglen - 1) / seglen;
    if (nseg64 > 0xffffffffull / no) return HH_ERR_UNSUPPORTED;
    const uint32_t nseg = (uint32_t)nseg64;
    const size_t nmap = (size_t)nseg * no;
    uint32_t *dm = nullptr;
    uint64_t *dbase = nullptr;
    uint32_t *hx = (uint32_t *)malloc(nmap * 8), *hent = (uint32_t *)malloc((size_t)nseg * 8);
    uint64_t *hbase = (uint64_t *)malloc((size_t)nseg * 8);
    int rc = HH_OK;
    if (!hx || !hent || !hbase) { rc = HH_ERR_NOMEM; goto out; }
    if (hipMalloc(&dm, nmap * 8 + (size_t)nseg * 8) != hipSuccess || hipMalloc(&dbase, (size_t)nseg * 8) != hipSuccess) {
        rc = HH_ERR_NOMEM;
        goto out;
    }
    {
        uint32_t *dexit = dm, *dcnt = dm + nmap;
        const uint64_t nl = nmap;
        hipLaunchKernelGGL(k_seg_func, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st,
                           (const uint32_t *)d_data, bits, seglen, nseg, no, d->tab, maxadv, dexit, dcnt);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(hx, dm, nmap * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { rc = HH_ERR_DEVICE; goto out; }
        const uint32_t *hexit = hx, *hcnt = hx + nmap;
        uint32_t o = 0;
        uint64_t run = 0;
        for (uint32_t sg = 0; sg < nseg; sg++) {
            if (o >= no) { rc = HH_ERR_INTERNAL; goto out; }
            hent[sg] = o;
            hent[nseg + sg] = hexit[(size_t)sg * no + o];
            hbase[sg] = run;
            run += hcnt[(size_t)sg * no + o];
            o = hent[nseg + sg];
        }
        *out_len = run;
        if (run > cap) { rc = HH_ERR_CAPACITY; goto out; }
        uint32_t *dent = dm;                            // (the maps are no longer needed)
        if (hipMemcpyAsync(dent, hent, (size_t)nseg * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(dbase, hbase, (size_t)nseg * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
            rc = HH_ERR_DEVICE;
            goto out;
        }
        hipLaunchKernelGGL(k_seg_emit, dim3((nseg + 255) / 256), dim3(256), 0, st, (const uint32_t *)d_data,
                           bits, seglen, nseg, d->tab, maxadv, dent, dent + nseg, dbase, d_out);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = HH_ERR_DEVICE;
    }
out:
    if (dm) hipFree(dm);
    if (dbase) hipFree(dbase);
    free(hx);
    free(hent);
    free(hbase);
    return rc;
}

// A complete fixed-length code: k_fixed (above).
// (ev: the events of the launch; wait = false: returns once enqueued)
int fixed_path(hh_decoder *d, const void *d_data, uint64_t bits, uint8_t *d_out, uint64_t cap,
               uint64_t *out_len, hipStream_t st, hipEvent_t *ev, bool wait) {
    if (!ev) ev = d->ev;
    const uint32_t L = d->fixed_len;
    const uint64_t nsym = bits / L + (bits % L ? 1 : 0);
    *out_len = nsym;
    d->stats.out_len = nsym;
    d->stats.fixed_length = 1;
    if (nsym > cap) return HH_ERR_CAPACITY;
    const uint64_t nthr = (nsym + 15) / 16, cap_blk = (uint64_t)(d->ncu ? d->ncu : 256) * 32;
    uint64_t nb = (nthr + 255) / 256;
    if (nb > cap_blk) nb = cap_blk;
    HIP_OK(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_fixed, dim3((unsigned)nb), dim3(256), 0, st, (const uint32_t *)d_data, bits, L,
                       (const uint8_t *)d->d_fsym, d->tab, d_out, nsym);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ev[3], st));
    if (!wait) return HH_OK;
    HIP_OK(hipEventSynchronize(ev[3]));
    float ms = 0;
    hipEventElapsedTime(&ms, ev[0], ev[3]);
    d->stats.ms_emit = ms;
    d->stats.ms_total = ms;
    return HH_OK;
}

// ---------------------------------------------------------------------------
// stage API
// ---------------------------------------------------------------------------
extern "C" int hh_stage_initbitsindex(hh_decoder *d, int32_t *idx, int64_t bits, void *s) {
    if (!d || !idx || bits < 0) return HH_ERR_ARG;
    hipLaunchKernelGGL(k_st_init, dim3(grid_for(bits, 256)), dim3(256), 0, (hipStream_t)s, idx, bits);
    HIP_OK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_stage_decodeallbits(hh_decoder *d, const void *data, int64_t bits,
                                      uint8_t *bitdecode, int32_t *steps, void *s) {
    if (!d || !d->have_tree || !data || !bitdecode || !steps || bits < 0) return HH_ERR_ARG;
    hipLaunchKernelGGL(k_st_decodeallbits, dim3(grid_for(bits, 256)), dim3(256), 0, (hipStream_t)s,
                       (const uint8_t *)data, bits, d->tab, bitdecode, steps);
    HIP_OK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_stage_makebigtable(hh_decoder *d, int64_t bits, int32_t *steps, int32_t step,
                                     int32_t *flag, void *s) {
    if (!d || !steps || step < 0 || step >= 24) return HH_ERR_ARG;
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(k_st_makebigtable, dim3(grid_for(bits, 256)), dim3(256), 0, st, bits, steps, step);
    HIP_OK(hipGetLastError());
    if (flag) {   // the reference's blocking 4-byte read (openclapproach.c:718-727)
        HIP_OK(hipMemcpyAsync(flag, steps + (int64_t)step * bits, 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    return HH_OK;
}

extern "C" int hh_stage_calcbitsindex(hh_decoder *d, int64_t bits, int32_t *idx, const int32_t *steps,
                                      int32_t step, int32_t pw, void *s) {
    if (!d || !idx || !steps || step < 1) return HH_ERR_ARG;
    hipLaunchKernelGGL(k_st_calcbitsindex, dim3(grid_for(bits, 256)), dim3(256), 0, (hipStream_t)s,
                       bits, idx, steps, step, pw);
    HIP_OK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_stage_calcresult(hh_decoder *d, int64_t bits, const int32_t *idx,
                                   const uint8_t *bitdecode, uint8_t *result, void *s) {
    if (!d || !idx || !bitdecode || !result) return HH_ERR_ARG;
    hipLaunchKernelGGL(k_st_calcresult, dim3(grid_for(bits, 256)), dim3(256), 0, (hipStream_t)s,
                       bits, idx, bitdecode, result, (uint64_t)bits);
    HIP_OK(hipGetLastError());
    return HH_OK;
}

extern "C" int hh_stage_findmax(hh_decoder *d, int64_t bits, const int32_t *idx, int32_t *maxvalue,
                                void *s) {
    if (!d || !idx || !maxvalue) return HH_ERR_ARG;
    hipStream_t st = (hipStream_t)s;
    HIP_OK(hipMemsetAsync(d->d_max, 0xff, 4, st));
    hipLaunchKernelGGL(k_st_findmax, dim3(grid_for(bits, 256)), dim3(256), 0, st, bits, idx, d->d_max);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(maxvalue, d->d_max, 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return HH_OK;
}

// The six stages driven like openclApproach (openclapproach.c:236-1047).
int stage_pipeline(hh_decoder *d, const void *d_data, int64_t bits, uint8_t *d_out,
                   uint64_t cap, uint64_t *out_len, hipStream_t st) {
    *out_len = 0;
    if (bits <= 0) return HH_OK;
    if (bits > 0x7fffffffLL) return HH_ERR_UNSUPPORTED;   // int32 arrays, as the reference
    uint8_t *bitdecode = nullptr, *result = nullptr;
    int32_t *steps = nullptr, *idx = nullptr;
    int rc = HH_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc(&bitdecode, bits) != hipSuccess || hipMalloc(&result, bits) != hipSuccess ||
        hipMalloc(&steps, (size_t)25 * bits * 4) != hipSuccess ||
        hipMalloc(&idx, (size_t)bits * 4) != hipSuccess) {
        rc = HH_ERR_NOMEM;
        goto done;
    }
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        rc = HH_ERR_DEVICE;
        goto done;
    }
    {
        hipEventRecord(e0, st);
        if ((rc = hh_stage_initbitsindex(d, idx, bits, st))) goto done;
        if ((rc = hh_stage_decodeallbits(d, d_data, bits, bitdecode, steps, st))) goto done;
        int32_t step = 0, flag = 0;
        do {
            if (step + 1 >= 25) { rc = HH_ERR_UNSUPPORTED; goto done; }
            if ((rc = hh_stage_makebigtable(d, bits, steps, step, &flag, st))) goto done;
            step++;
        } while (flag != -1);
        int32_t pw = 1 << (step - 1);
        const int32_t zero = 0;
        if (hipMemcpyAsync(idx, &zero, 4, hipMemcpyHostToDevice, st) != hipSuccess) {
            rc = HH_ERR_DEVICE;
            goto done;
        }
        while (step > 0) {
            if ((rc = hh_stage_calcbitsindex(d, bits, idx, steps, step, pw, st))) goto done;
            step--;
            pw >>= 1;
        }
        if ((rc = hh_stage_calcresult(d, bits, idx, bitdecode, result, st))) goto done;
        int32_t mx = -1;
        if ((rc = hh_stage_findmax(d, bits, idx, &mx, st))) goto done;
        uint64_t n = (uint64_t)mx + 1;
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        d->stats.ms_total = ms;
        d->stats.out_len = n;
        *out_len = n;
        if (n > cap) { rc = HH_ERR_CAPACITY; goto done; }
        if (n && hipMemcpyAsync(d_out, result, n, hipMemcpyDeviceToDevice, st) != hipSuccess)
            rc = HH_ERR_DEVICE;
        if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = HH_ERR_DEVICE;
    }
done:
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    hipFree(bitdecode);
    hipFree(result);
    hipFree(steps);
    hipFree(idx);
    return rc;
}

extern "C" int hh_stage_pipeline(hh_decoder *d, const void *d_data, int64_t bits, uint8_t *d_out,
                                 uint64_t cap, uint64_t *out_len, void *s) {
    if (!d || !d->have_tree || !out_len) return HH_ERR_ARG;
    HIP_OK(hipSetDevice(d->device));
    hipStream_t st = (hipStream_t)s;   // NULL = the default stream
    return stage_pipeline(d, d_data, bits, d_out, cap, out_len, st);
}
