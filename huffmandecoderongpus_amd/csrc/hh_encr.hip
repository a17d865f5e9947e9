// Ragged blocked device encoder: n symbols cut into nrec records at a device
// list of offsets (offs[0] = 0 <= ... <= offs[nrec] = n), every record its own
// LSB-first stream from the root (as hh_encode of those symbols alone), the
// streams packed at 4-byte boundaries; an empty record takes no bytes.  The
// producer of hh_decode_batch_device(_items) for records of any lengths.
//
// The text is cut into chunks of ENC_CH symbols whatever the records do: a
// workgroup's 4096 symbols hold as many records as fall into them, and every
// step over the records is a thread per record on as many workgroups as they
// need (rules: hh_encr_algo.h).  P(i): the exclusive prefix of the code
// lengths; symbol i of record r lands at output bit 32 wb[r] + P(i) -
// P(offs[r]).  Launches, all on the caller's stream:
//   k_encr_cut     a thread per chunk edge: rlo[c], the first record that
//                  starts at or after symbol c ENC_CH (one binary search each,
//                  all at once, instead of two per workgroup of the next pass
//                  one after the other);
//   k_encr_len     a workgroup per chunk: its bits, the absent-symbol flag,
//                  and for every record that starts in it, rlo[c] ..
//                  rlo[c + 1], loc[r] = the bits of the chunk before symbol
//                  offs[r] (from the symbols' prefixes in LDS, a thread per
//                  record);
//   k_encr_csums, k_encr_cfirst   the chunks' bits into exclusive offsets CS,
//                  tiles of 1024: a workgroup per tile for its sum, then one
//                  per tile again, which adds up the tiles before it itself
//                  (at most 2^14 of them);
//   k_encr_rsums   a thread per record: the offsets check, start[r] =
//                  CS[offs[r] / 4096] + loc[r] (the total at the text's end),
//                  bits[r] = start[r + 1] - start[r], the tile's words;
//   k_encr_top, k_encr_rfirst   those into wb[r]: one workgroup over the tile
//                  sums with the carry, then a workgroup per tile;
//   k_encr_items   a thread per record: the hh_batch_item list;
//   (the host reads totals and flags, checks the capacity, zeroes the output)
//   k_encr_pack    a workgroup per chunk: the chunk's image in LDS from the
//                  output word of its first symbol to that of its last,
//                  k_encb_pack's body with the position formula above; plain
//                  stores inside, atomic ORs on the first and the last word.
// No workgroup loops over all records: k_encr_top steps through their tile
// sums, 1024 tiles (2^20 records) a step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "hiphuff.h"
#include "hh_internal.h"
#include "hh_enc.h"
#include "hh_enc_kern.h"
#include "hh_encr_algo.h"

static_assert(HER_CH == ENC_CH && HER_TILE == ENC_SCAN_TB, "hh_encr_algo.h restates the encoder's geometry");

__global__ __launch_bounds__(ENC_TB) void k_encr_cut(const uint64_t *__restrict__ offs, uint64_t nrec, uint64_t n,
                                                     uint32_t nch, uint32_t *__restrict__ rlo) {
    const uint64_t c = (uint64_t)blockIdx.x * ENC_TB + threadIdx.x;
    if (c > nch) return;
    const uint64_t t = c * ENC_CH < n ? c * ENC_CH : n;
    rlo[c] = (uint32_t)her_lower(offs, nrec, t);          // (nrec < 2^32 - 1)
}

// The inclusive prefix of v over the ENC_TB threads; *tot the workgroup's sum.
__device__ __forceinline__ uint32_t encr_scan256(uint32_t v, uint32_t *s_w, uint32_t *tot) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t base = 0, t = 0;
#pragma unroll
    for (uint32_t i = 0; i < ENC_TB / 64; i++) {
        base += i < wv ? s_w[i] : 0u;
        t += s_w[i];
    }
    *tot = t;
    return base + x;
}

__global__ __launch_bounds__(ENC_TB) void k_encr_len(const uint8_t *__restrict__ syms, uint64_t n,
                                                     const EncTab *__restrict__ tab, const uint64_t *__restrict__ offs,
                                                     const uint32_t *__restrict__ rlo, uint64_t *__restrict__ csum,
                                                     uint32_t *__restrict__ loc, uint32_t *flags) {
    __shared__ __align__(16) uint32_t s_pre[ENC_CH];
    __shared__ uint32_t s_len[256];
    __shared__ uint32_t s_w[ENC_TB / 64];
    const uint32_t tid = threadIdx.x;
    s_len[tid] = tab->len[tid];
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * ENC_CH, c1 = n - c0 < ENC_CH ? n : c0 + ENC_CH;
    const uint64_t i0 = c0 + (uint64_t)tid * ENC_PT;
    uint8_t sy[ENC_PT];
    enc_load16(syms, c1, i0, sy);
    uint32_t l[ENC_PT], sum = 0;
    bool miss = false;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) {
        l[k] = 0;
        if (i0 + k < c1) {
            l[k] = s_len[sy[k]];
            miss |= l[k] == 0;
        }
        sum += l[k];
    }
    uint32_t tot;
    const uint32_t x = encr_scan256(sum, s_w, &tot);
    if (tid == 0) csum[blockIdx.x] = tot;
    if (miss) atomicOr(flags, HER_F_ABSENT);
    // the records that start in this chunk (none in most chunks of long records)
    const uint32_t r0 = rlo[blockIdx.x], r1 = rlo[blockIdx.x + 1];
    if (r0 >= r1) return;                                     // (the whole workgroup)
    uint32_t p = x - sum;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) {
        s_pre[tid * ENC_PT + k] = p;
        p += l[k];
    }
    __syncthreads();
    const uint64_t cnt = c1 - c0;
    bool bad = false;
    for (uint64_t r = (uint64_t)r0 + tid; r < r1; r += ENC_TB) {
        const uint64_t o = offs[r] - c0;
        if (o < cnt) loc[r] = s_pre[o];
        else bad = true;                                      // (offs is not sorted)
    }
    if (bad) atomicOr(flags, HER_F_OFFS);
}

// One tile of ENC_SCAN_TB values: this thread's inclusive prefix within the
// workgroup, *tot the tile's sum.
__device__ __forceinline__ uint64_t encr_scan_tile(uint64_t v, uint64_t *s_w, uint64_t *tot) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint64_t base = 0, t = 0;
    for (uint32_t i = 0; i < ENC_SCAN_TB / 64; i++) {
        base += i < wv ? s_w[i] : 0;
        t += s_w[i];
    }
    __syncthreads();
    *tot = t;
    return base + x;
}

// One workgroup: nt tile sums into exclusive ones in place, ENC_SCAN_TB a
// step with the carry; *total their sum.
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_top(uint64_t *__restrict__ sums, uint64_t nt,
                                                          uint64_t *__restrict__ total) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    uint64_t carry = 0, tot;
    for (uint64_t t0 = 0; t0 < nt; t0 += ENC_SCAN_TB) {
        const uint64_t t = t0 + threadIdx.x;
        const uint64_t v = t < nt ? sums[t] : 0;
        const uint64_t x = encr_scan_tile(v, s_w, &tot);
        if (t < nt) sums[t] = carry + x - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// A workgroup per tile of chunks: the tile's bits.
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_csums(const uint64_t *__restrict__ csum, uint64_t nch,
                                                            uint64_t *__restrict__ ctile) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    const uint64_t c = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    uint64_t tot;
    (void)encr_scan_tile(c < nch ? csum[c] : 0, s_w, &tot);
    if (threadIdx.x == 0) ctile[blockIdx.x] = tot;
}

// A workgroup per tile of chunks: CS[c] the chunks' bits on entry, their
// exclusive offsets on return, CS[nch] the total, which the last workgroup
// also leaves in *total.  The tile's base is the sum of the tiles before it,
// which every workgroup adds up for itself: a launch's grid holds fewer than
// 2^24 chunks, 2^14 tiles, 16 values a thread at the most -- no pass of one
// workgroup over the tile sums at this level.
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_cfirst(uint64_t *__restrict__ CS, uint64_t nch,
                                                             const uint64_t *__restrict__ ctile,
                                                             uint64_t *__restrict__ total) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    uint64_t before = 0, base, tot;
    for (uint32_t t = threadIdx.x; t < blockIdx.x; t += ENC_SCAN_TB) before += ctile[t];
    (void)encr_scan_tile(before, s_w, &base);
    const uint64_t c = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    const uint64_t v = c < nch ? CS[c] : 0;
    const uint64_t x = encr_scan_tile(v, s_w, &tot);
    if (c <= nch) CS[c] = base + x - v;
    if (c == nch) *total = base + x;
}

// A thread per record: the offsets' rules, start[r], bits[r], and the tile's
// output words.  res[0]: the total bits (k_encr_top over the chunks).
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_rsums(const uint64_t *__restrict__ offs, uint64_t nrec,
                                                            uint64_t n, const uint64_t *__restrict__ CS,
                                                            const uint32_t *__restrict__ loc,
                                                            const uint64_t *__restrict__ res,
                                                            uint64_t *__restrict__ start, uint64_t *__restrict__ bits,
                                                            uint64_t *__restrict__ rtile, uint32_t *flags) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    const uint64_t r = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    uint64_t w = 0;
    if (r < nrec) {
        const uint64_t a = offs[r], b = offs[r + 1];
        const bool ok = her_pair_ok(a, b, n) && (r != 0 || a == 0) && (r + 1 != nrec || b == n);
        uint64_t s0 = 0, s1 = 0;
        if (ok) {
            // (a <= b <= n, and b < n only before the last record: loc[r + 1] exists)
            const uint64_t total = res[0];
            s0 = her_start(CS, a, a == n ? 0u : loc[r], n, total);
            s1 = her_start(CS, b, b == n ? 0u : loc[r + 1], n, total);
        } else {
            atomicOr(flags, HER_F_OFFS);
        }
        start[r] = s0;
        bits[r] = s1 - s0;
        w = her_words(s1 - s0);
    }
    uint64_t tot;
    (void)encr_scan_tile(w, s_w, &tot);
    if (threadIdx.x == 0) rtile[blockIdx.x] = tot;
}

__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_rfirst(const uint64_t *__restrict__ bits, uint64_t nrec,
                                                             const uint64_t *__restrict__ rtile,
                                                             uint64_t *__restrict__ wb) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    const uint64_t r = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    const uint64_t v = r < nrec ? her_words(bits[r]) : 0;
    uint64_t tot;
    const uint64_t x = encr_scan_tile(v, s_w, &tot);
    if (r < nrec) wb[r] = rtile[blockIdx.x] + x - v;
}

// The items from the scan's arrays, a thread per record; none when a flag is
// up (the arrays mean nothing then).
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encr_items(const uint64_t *__restrict__ offs,
                                                            const uint64_t *__restrict__ bits,
                                                            const uint64_t *__restrict__ wb, uint64_t nrec,
                                                            const uint32_t *__restrict__ flags,
                                                            hh_batch_item *__restrict__ items) {
    const uint64_t r = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    if (r >= nrec || *flags) return;
    const uint64_t a = offs[r];
    items[r] = hh_batch_item{4u * wb[r], bits[r], a, offs[r + 1] - a};
}

// Runs only after the host has seen the flag word clear (offs keeps its rules,
// every symbol has a code) and zeroed the output.  s_img holds first the
// chunk's record marks -- mark[o] = 1 + the last record that starts at symbol
// c0 + o, the non-empty one of a run of empties -- which every thread takes
// into registers; then the image.  img_alloc: the dynamic LDS in words, at
// least ENC_CH.
__global__ __launch_bounds__(ENC_TB) void k_encr_pack(const uint8_t *__restrict__ syms, uint64_t n,
                                                      const EncTab *__restrict__ tab,
                                                      const uint64_t *__restrict__ offs,
                                                      const uint32_t *__restrict__ rlo, const uint64_t *__restrict__ CS,
                                                      const uint64_t *__restrict__ start,
                                                      const uint64_t *__restrict__ wb, uint32_t *__restrict__ out,
                                                      uint64_t total_words, uint32_t img_alloc, uint32_t *flags) {
    extern __shared__ __align__(16) uint32_t s_img[];
    __shared__ uint64_t s_code[256];
    __shared__ uint32_t s_len[256];
    __shared__ uint32_t s_w[ENC_TB / 64], s_m[ENC_TB / 64], s_m0;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t c0 = (uint64_t)blockIdx.x * ENC_CH, c1 = n - c0 < ENC_CH ? n : c0 + ENC_CH;
    const uint64_t cnt = c1 - c0;
    const uint32_t r0 = rlo[blockIdx.x], r1 = rlo[blockIdx.x + 1];
    s_code[tid] = tab->code[tid];
    s_len[tid] = tab->len[tid];
    for (uint32_t i = tid; i < ENC_CH; i += ENC_TB) s_img[i] = 0u;
    __syncthreads();
    for (uint64_t r = (uint64_t)r0 + tid; r < r1; r += ENC_TB) {
        const uint64_t o = offs[r] - c0;
        if (o < cnt) atomicMax(&s_img[o], (uint32_t)r + 1u);
    }
    __syncthreads();
    uint32_t m[ENC_PT], tm = 0;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) {
        m[k] = s_img[tid * ENC_PT + k];
        tm = tm > m[k] ? tm : m[k];
    }
    // this thread's symbols and their bits
    const uint64_t i0 = c0 + (uint64_t)tid * ENC_PT;
    uint8_t sy[ENC_PT];
    enc_load16(syms, c1, i0, sy);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) sum += i0 + k < c1 ? s_len[sy[k]] : 0u;
    // the threads' bits and marks: the inclusive sum and the inclusive maximum
    uint32_t x = sum, mx = tm;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64), z = __shfl_up(mx, o, 64);
        if (lane >= (uint32_t)o) {
            x += y;
            mx = mx > z ? mx : z;
        }
    }
    if (lane == 63) {
        s_w[wv] = x;
        s_m[wv] = mx;
    }
    if (tid == 0) s_m0 = m[0];
    uint32_t em = __shfl_up(mx, 1, 64);                       // (the mark in force at this thread's first symbol)
    if (lane == 0) em = 0u;
    __syncthreads();                                          // (every mark is in registers: s_img is free)
    uint32_t base = 0;
#pragma unroll
    for (uint32_t i = 0; i < ENC_TB / 64; i++) {
        base += i < wv ? s_w[i] : 0u;
        em = i < wv && s_m[i] > em ? s_m[i] : em;
    }
    // the chunk's first and last record, the image they span: the one in
    // force at its first symbol (r0 - 1 runs on from the chunk before unless
    // one starts there), and the last that starts before its end
    const uint32_t mark0 = s_m0;
    if (r1 == 0 || (mark0 == 0 && r0 == 0)) {                 // (never with offs[0] == 0; the whole workgroup)
        if (tid == 0) atomicOr(flags, HER_F_INTERNAL);
        return;
    }
    const uint32_t rf = mark0 ? mark0 - 1u : r0 - 1u, rl = r1 - 1u;
    const uint64_t CSc = CS[blockIdx.x];
    const uint64_t g0 = her_pos(wb[rf], start[rf], CSc), gend = her_pos(wb[rl], start[rl], CS[blockIdx.x + 1]);
    const uint64_t W0 = g0 >> 5;
    const uint64_t nw64 = gend > g0 ? her_img_words(g0, gend) : 0;
    if (nw64 == 0 || nw64 > img_alloc || W0 + nw64 > total_words || W0 + nw64 < W0) {
        if (tid == 0) atomicOr(flags, HER_F_INTERNAL);
        return;
    }
    const uint32_t nw = (uint32_t)nw64;
    for (uint32_t i = tid; i < nw; i += ENC_TB) s_img[i] = 0u;
    __syncthreads();
    // each code's bits ORed into its (up to three) image words
    uint32_t cur = em ? em - 1u : r0 - 1u;
    uint64_t wbc = 0, stc = 0;
    if (i0 < c1 && !m[0]) {
        wbc = wb[cur];
        stc = start[cur];
    }
    uint64_t P = CSc + (base + x - sum);
    bool over = false;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) {
        if (i0 + k >= c1) break;
        if (m[k]) {                                           // (i == offs[r]: the next record, over empties too)
            cur = m[k] - 1u;
            wbc = wb[cur];
            stc = start[cur];
        }
        const uint32_t l = s_len[sy[k]];
        const uint64_t c = s_code[sy[k]];
        const uint64_t g = her_pos(wbc, stc, P) - 32u * W0;
        P += l;
        if (g + l > 32ull * nw) {                             // (never: the image spans the chunk's bits)
            over = true;
            continue;
        }
        const uint32_t p = (uint32_t)g;
        const uint32_t w = p >> 5, o = p & 31u;
        const uint64_t v = c << o;
        if (l) atomicOr(&s_img[w], (uint32_t)v);
        if (o + l > 32u) atomicOr(&s_img[w + 1], (uint32_t)(v >> 32));
        if (o + l > 64u) atomicOr(&s_img[w + 2], (uint32_t)(c >> (64u - o)));
    }
    if (over) atomicOr(flags, HER_F_INTERNAL);
    __syncthreads();
    // out: symbol order is output order, so a word strictly inside the image
    // is this chunk's alone; its first and last word may be a neighbour's too
    uint32_t *dst = out + W0;
    for (uint32_t i = tid; i < nw; i += ENC_TB) {
        if (i == 0 || i + 1 == nw) atomicOr(dst + i, s_img[i]);
        else dst[i] = s_img[i];
    }
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// hh_encoder_encode_ragged; *total_bits (may be NULL) for the compress check.
static int encode_ragged(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n, const uint64_t *d_offs,
                         uint64_t nrec, void *d_out, uint64_t cap, hh_batch_item *d_items, hh_batch_item *items,
                         uint64_t *total_bytes, uint64_t *total_bits, void *hip_stream) {
    if (!enc || !tree || !total_bytes || (!d_out && cap)) return HH_ERR_ARG;
    if ((n && !d_syms) || (nrec && !d_offs)) return HH_ERR_ARG;
    if (((uintptr_t)d_offs & 7u) != 0 || ((uintptr_t)d_items & 7u) != 0) return HH_ERR_ARG;  // (64-bit loads, stores)
    if (((uintptr_t)d_out & 3u) != 0) return HH_ERR_ARG;   // (32-bit word stores)
    *total_bytes = 0;
    if (total_bits) *total_bits = 0;
    EncTab h;
    uint8_t len8[256];
    int rc = hh_codebook(tree, h.code, len8);
    if (rc) return rc;
    uint32_t maxlen = 0;
    for (int i = 0; i < 256; i++) {
        h.len[i] = len8[i];
        maxlen = len8[i] > maxlen ? len8[i] : maxlen;
    }
    if (nrec >= 0xffffffffull) return HH_ERR_UNSUPPORTED;
    const uint64_t nch = n / ENC_CH + (n % ENC_CH != 0);
    // (a launch's grid may not exceed 2^32 - 1 threads: about 2^24 chunks)
    if (nch * ENC_TB > 0xffffffffull) return HH_ERR_UNSUPPORTED;
    if (nrec == 0) return n == 0 ? HH_OK : HH_ERR_ARG;      // (offs[0] is not both 0 and n)
    if (hipSetDevice(enc->device) != hipSuccess) return HH_ERR_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t ntc = nch / ENC_SCAN_TB + 1, ntr = (nrec + ENC_SCAN_TB - 1) / ENC_SCAN_TB;
    hh_batch_item *d_it = d_items;
    const size_t o_rlo = al256(sizeof(EncTab)), o_cs = o_rlo + al256((nch + 1) * 4),
                 o_loc = o_cs + al256((nch + 1) * 8), o_start = o_loc + al256(nrec * 4), o_bits = o_start + al256(nrec * 8),
                 o_wb = o_bits + al256(nrec * 8), o_it = o_wb + al256(nrec * 8),
                 o_ct = o_it + (items && !d_items ? al256(nrec * sizeof(hh_batch_item)) : 0),
                 o_rt = o_ct + al256(ntc * 8), o_res = o_rt + al256(ntr * 8), need = o_res + 64;
    if (enc->size < need) {
        // (the previous call on this encoder has returned: its stream is done
        // with the old workspace, no device-wide wait)
        if (enc->ws) (void)hipFree(enc->ws);
        enc->ws = nullptr;
        enc->size = 0;
        if (hipMalloc(&enc->ws, need) != hipSuccess) return HH_ERR_NOMEM;
        enc->size = need;
    }
    uint8_t *ws = enc->ws;
    EncTab *d_tab = (EncTab *)ws;
    uint32_t *d_rlo = (uint32_t *)(ws + o_rlo), *d_loc = (uint32_t *)(ws + o_loc);
    uint64_t *d_cs = (uint64_t *)(ws + o_cs), *d_start = (uint64_t *)(ws + o_start),
             *d_bits = (uint64_t *)(ws + o_bits), *d_wb = (uint64_t *)(ws + o_wb), *d_ct = (uint64_t *)(ws + o_ct),
             *d_rt = (uint64_t *)(ws + o_rt), *d_res = (uint64_t *)(ws + o_res);
    uint32_t *d_flags = (uint32_t *)(ws + o_res + 32);
    if (items && !d_items) d_it = (hh_batch_item *)(ws + o_it);
    const uint32_t img_alloc = her_img_alloc(maxlen, nrec) > ENC_CH ? her_img_alloc(maxlen, nrec) : ENC_CH;
    uint64_t hres[5] = {0, 0, 0, 0, 0};
    uint32_t hflags = 0;
    rc = HH_ERR_DEVICE;
    do {
        if (hipMemcpyAsync(d_tab, &h, sizeof(h), hipMemcpyHostToDevice, st) != hipSuccess) break;
        // (the tile sums, the totals, the flags)
        if (hipMemsetAsync(ws + o_ct, 0, need - o_ct, st) != hipSuccess) break;
        if (nch) {
            hipLaunchKernelGGL(k_encr_cut, dim3((unsigned)(nch / ENC_TB + 1)), dim3(ENC_TB), 0, st, d_offs, nrec, n,
                               (uint32_t)nch, d_rlo);
            if (hipGetLastError() != hipSuccess) break;
            hipLaunchKernelGGL(k_encr_len, dim3((unsigned)nch), dim3(ENC_TB), 0, st, (const uint8_t *)d_syms, n, d_tab,
                               d_offs, d_rlo, d_cs, d_loc, d_flags);
            if (hipGetLastError() != hipSuccess) break;
        }
        hipLaunchKernelGGL(k_encr_csums, dim3((unsigned)ntc), dim3(ENC_SCAN_TB), 0, st, d_cs, nch, d_ct);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_encr_cfirst, dim3((unsigned)ntc), dim3(ENC_SCAN_TB), 0, st, d_cs, nch, d_ct, d_res);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_encr_rsums, dim3((unsigned)ntr), dim3(ENC_SCAN_TB), 0, st, d_offs, nrec, n, d_cs, d_loc,
                           d_res, d_start, d_bits, d_rt, d_flags);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_encr_top, dim3(1), dim3(ENC_SCAN_TB), 0, st, d_rt, ntr, d_res + 1);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_encr_rfirst, dim3((unsigned)ntr), dim3(ENC_SCAN_TB), 0, st, d_bits, nrec, d_rt, d_wb);
        if (hipGetLastError() != hipSuccess) break;
        if (d_it) {
            hipLaunchKernelGGL(k_encr_items, dim3((unsigned)ntr), dim3(ENC_SCAN_TB), 0, st, d_offs, d_bits, d_wb, nrec,
                               d_flags, d_it);
            if (hipGetLastError() != hipSuccess) break;
        }
        if (hipMemcpyAsync(hres, d_res, 40, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        if (hipStreamSynchronize(st) != hipSuccess) break;
        hflags = (uint32_t)hres[4];
        if (hflags & HER_F_INTERNAL) { rc = HH_ERR_INTERNAL; break; }
        if (hflags) { rc = HH_ERR_ARG; break; }              // (offs breaks a rule, or a symbol absent from the tree)
        if (items && hipMemcpyAsync(items, d_it, nrec * sizeof(hh_batch_item), hipMemcpyDeviceToHost, st) != hipSuccess)
            break;
        if (hres[1] > ~0ull / 4 || hres[1] * 32 < hres[0]) { rc = HH_ERR_INTERNAL; break; }
        const uint64_t off = hres[1] * 4;
        *total_bytes = off;
        if (total_bits) *total_bits = hres[0];
        if (off > cap) {
            rc = hipStreamSynchronize(st) == hipSuccess ? HH_ERR_CAPACITY : HH_ERR_DEVICE;
            break;
        }
        if (off) {
            if (hipMemsetAsync(d_out, 0, off, st) != hipSuccess) break;
            hipLaunchKernelGGL(k_encr_pack, dim3((unsigned)nch), dim3(ENC_TB), (size_t)img_alloc * 4, st,
                               (const uint8_t *)d_syms, n, d_tab, d_offs, d_rlo, d_cs, d_start, d_wb, (uint32_t *)d_out,
                               hres[1], img_alloc, d_flags);
            if (hipGetLastError() != hipSuccess) break;
            if (hipMemcpyAsync(&hflags, d_flags, 4, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        }
        if (hipStreamSynchronize(st) != hipSuccess) break;
        rc = hflags ? HH_ERR_INTERNAL : HH_OK;
    } while (0);
    if (rc != HH_OK && rc != HH_ERR_CAPACITY) *total_bytes = 0;
    return rc;
}

extern "C" int hh_encoder_encode_ragged(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                                        const uint64_t *d_offs, uint64_t nrec, void *d_out, uint64_t cap,
                                        hh_batch_item *d_items, hh_batch_item *items, uint64_t *total_bytes,
                                        void *hip_stream) {
    return encode_ragged(enc, tree, d_syms, n, d_offs, nrec, d_out, cap, d_items, items, total_bytes, nullptr,
                         hip_stream);
}

// The bound: hh_compress_blocks_bound's argument with nrec for the blocks --
// all the records together are the text under the Huffman code of its own
// counts, at most 8 n bits, and a record of bits[r] bits takes less than
// bits[r] / 8 + 4 bytes (an empty one none).
extern "C" uint64_t hh_compress_ragged_bound(uint64_t n, uint64_t nrec) { return (n + 3) / 4 * 4 + 4 * nrec; }

// Compress into records: one histogram of all n bytes and one tree for all
// the records, then the ragged encode; its total bits must be the
// histogram's sum of count x code length.
extern "C" int hh_compress_ragged_device(hh_encoder *enc, const void *d_syms, uint64_t n, const uint64_t *d_offs,
                                         uint64_t nrec, void *d_out, uint64_t cap, hh_tree_buf *tree,
                                         hh_batch_item *d_items, hh_batch_item *items, uint64_t *total_bytes,
                                         void *hip_stream) {
    if (!enc || !d_syms || !d_offs || !tree || !total_bytes || n == 0 || nrec == 0 || (!d_out && cap))
        return HH_ERR_ARG;
    if (((uintptr_t)d_out & 3u) != 0) return HH_ERR_ARG;   // (32-bit word stores)
    *total_bytes = 0;
    uint64_t counts[256];
    int rc = hh_histogram_device(enc, d_syms, n, counts, hip_stream);
    if (rc) return rc;
    rc = hh_tree_build(counts, tree);
    if (rc) return rc;
    const hh_tree t = {tree->nodes, tree->izero, tree->ione, tree->sym};
    uint64_t code[256];
    uint8_t len8[256];
    rc = hh_codebook(&t, code, len8);
    if (rc) return rc;
    uint64_t pred = 0, got = 0;
    for (int s = 0; s < 256; s++) pred += counts[s] * len8[s];   // (<= 64 n < 2^43)
    rc = encode_ragged(enc, &t, d_syms, n, d_offs, nrec, d_out, cap, d_items, items, total_bytes, &got, hip_stream);
    if (rc != HH_OK && rc != HH_ERR_CAPACITY) return rc;
    if (got != pred) return HH_ERR_INTERNAL;
    return rc;
}
