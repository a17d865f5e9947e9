// Blocked device encoder: n symbols cut into blocks of block_syms, every
// block its own LSB-first stream from the root (as hh_encode of those symbols
// alone), the streams packed at 4-byte boundaries -- the producer of what
// hh_decode_batch_device (csrc/hh_batch.hip) takes.  The single-stream
// encoder's geometry (csrc/hh_encode.hip, hh_enc_kern.h) with pieces for
// chunks: a block is cut into pieces of ENC_CH symbols, the last one shorter,
// so that a piece never straddles a block; every block has ppb =
// ceil(block_syms / ENC_CH) piece slots (the last block's unused ones are
// empty), piece p belongs to block p / ppb.  Three launches on the caller's
// stream:
//   k_encb_len   one workgroup per piece: its code bits (and whether a symbol
//                is absent from the tree);
//   k_encb_scan  one workgroup, two levels: the exclusive scan S of the
//                pieces' bits; then, per block b, bits[b] = S[(b + 1) ppb] -
//                S[b ppb] and the exclusive scan wb of ceil(bits[b] / 32),
//                the block's first output word -- the round-up at every block
//                end.  No thread loops over a block's pieces;
//   k_encb_pack  one workgroup per piece, as k_enc_pack: the piece's image in
//                LDS from bit 32 wb[b] + S[p] - S[b ppb], plain stores inside,
//                atomic ORs on its first and last word (pieces of one block
//                share words, blocks never do; the output is zeroed first).
// The blocks' bits, the totals and the flag come back in copies on the same
// stream; the host fills the hh_batch_item list.  The _items entries also
// leave that list on the device (k_encb_items, after the scan), where
// hh_decode_batch_device_items takes it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "hiphuff.h"
#include "hh_internal.h"
#include "hh_enc.h"
#include "hh_enc_kern.h"

// Piece p: the symbols [*i0, *i1) (empty for the last block's unused slots).
__device__ __forceinline__ void encb_piece(uint32_t p, uint32_t ppb, uint64_t n, uint64_t block_syms, uint64_t *i0,
                                           uint64_t *i1) {
    const uint32_t b = p / ppb, j = p - b * ppb;
    const uint64_t bs = (uint64_t)b * block_syms;
    const uint64_t be = n - bs < block_syms ? n : bs + block_syms;      // (bs < n: b < nb)
    const uint64_t s = bs + (uint64_t)j * ENC_CH;
    *i0 = s < be ? s : be;
    *i1 = be - *i0 < ENC_CH ? be : *i0 + ENC_CH;
}

__global__ __launch_bounds__(ENC_TB) void k_encb_len(const uint8_t *__restrict__ syms, uint64_t n, uint64_t block_syms,
                                                     uint32_t ppb, const EncTab *__restrict__ tab,
                                                     uint64_t *__restrict__ pbits, uint32_t *__restrict__ bad) {
    __shared__ uint32_t s_len[256];
    __shared__ uint32_t s_w[ENC_TB / 64];
    const uint32_t tid = threadIdx.x;
    s_len[tid] = tab->len[tid];
    __syncthreads();
    uint64_t p0, p1;
    encb_piece(blockIdx.x, ppb, n, block_syms, &p0, &p1);
    const uint64_t i0 = p0 + (uint64_t)tid * ENC_PT;
    uint8_t sy[ENC_PT];
    enc_load16(syms, p1, i0, sy);
    uint32_t sum = 0;
    bool miss = false;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++)
        if (i0 + k < p1) {
            const uint32_t l = s_len[sy[k]];
            sum += l;
            miss |= l == 0;
        }
    const uint32_t tot = enc_block_sum(sum, s_w);
    if (tid == 0) pbits[blockIdx.x] = tot;
    if (miss) atomicOr(bad, 1u);
}

// One tile of ENC_SCAN_TB values: this thread's inclusive prefix within the
// workgroup, *tot the tile's sum.
__device__ __forceinline__ uint64_t encb_scan_tile(uint64_t v, uint64_t *s_w, uint64_t *tot) {
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

// One workgroup.  S: npc pieces' bits -> their exclusive offsets (in place),
// S[npc] the total; then the blocks: bbits[b], wb[b] the block's first output
// word.  res[0] the total bits, res[1] the total words.
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encb_scan(uint64_t *S, uint64_t npc, uint32_t ppb, uint64_t nb,
                                                           uint64_t *__restrict__ bbits, uint64_t *__restrict__ wb,
                                                           uint64_t *__restrict__ res) {
    __shared__ uint64_t s_w[ENC_SCAN_TB / 64];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0, tot;
    for (uint64_t p0 = 0; p0 < npc; p0 += ENC_SCAN_TB) {
        const uint64_t v = p0 + tid < npc ? S[p0 + tid] : 0;
        const uint64_t x = encb_scan_tile(v, s_w, &tot);
        if (p0 + tid < npc) S[p0 + tid] = carry + x - v;
        carry += tot;
    }
    if (tid == 0) {
        S[npc] = carry;
        res[0] = carry;
    }
    __threadfence();
    __syncthreads();        // (S is read back below by other threads of this workgroup)
    carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += ENC_SCAN_TB) {
        const uint64_t b = b0 + tid;
        uint64_t bits = 0;
        if (b < nb) bits = S[(b + 1) * ppb] - S[b * ppb];
        const uint64_t v = (bits + 31) / 32;
        const uint64_t x = encb_scan_tile(v, s_w, &tot);
        if (b < nb) {
            bbits[b] = bits;
            wb[b] = carry + x - v;
        }
        carry += tot;
    }
    if (tid == 0) res[1] = carry;
}

__global__ __launch_bounds__(ENC_TB) void k_encb_pack(const uint8_t *__restrict__ syms, uint64_t n, uint64_t block_syms,
                                                      uint32_t ppb, const EncTab *__restrict__ tab,
                                                      const uint64_t *__restrict__ S, const uint64_t *__restrict__ wb,
                                                      uint32_t *__restrict__ out) {
    extern __shared__ __align__(16) uint32_t s_img[];
    __shared__ uint64_t s_code[256];
    __shared__ uint32_t s_len[256];
    __shared__ uint32_t s_w[ENC_TB / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    // the piece: its symbols, its first bit in the output and its bit count
    const uint32_t pc = blockIdx.x, b = pc / ppb;
    const uint64_t sb = S[pc], nbits = S[pc + 1] - sb;
    if (nbits == 0) return;                                  // (an empty slot; the whole workgroup)
    s_code[tid] = tab->code[tid];
    s_len[tid] = tab->len[tid];
    const uint64_t gb = 32u * wb[b] + (sb - S[(uint64_t)b * ppb]);
    const uint32_t sh0 = (uint32_t)(gb & 31u);
    const uint32_t nw = (uint32_t)((sh0 + nbits + 31u) / 32u);
    for (uint32_t i = tid; i < nw; i += ENC_TB) s_img[i] = 0u;
    __syncthreads();
    // this thread's symbols and their bits; the end it tests against is the piece's
    uint64_t p0, p1;
    encb_piece(pc, ppb, n, block_syms, &p0, &p1);
    const uint64_t i0 = p0 + (uint64_t)tid * ENC_PT;
    uint8_t sy[ENC_PT];
    enc_load16(syms, p1, i0, sy);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) sum += i0 + k < p1 ? s_len[sy[k]] : 0u;
    // exclusive scan of the threads' bits within the piece
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (uint32_t i = 0; i < ENC_TB / 64; i++) base += i < wv ? s_w[i] : 0u;
    uint32_t p = sh0 + base + x - sum;     // (bit position in the image)
    // each code's bits ORed into its (up to three) image words
#pragma unroll
    for (uint32_t k = 0; k < ENC_PT; k++) {
        if (i0 + k >= p1) break;
        const uint32_t l = s_len[sy[k]];
        const uint64_t c = s_code[sy[k]];
        const uint32_t w = p >> 5, o = p & 31u;
        const uint64_t v = c << o;
        if (l) atomicOr(&s_img[w], (uint32_t)v);
        if (o + l > 32u) atomicOr(&s_img[w + 1], (uint32_t)(v >> 32));
        if (o + l > 64u) atomicOr(&s_img[w + 2], (uint32_t)(c >> (64u - o)));
        p += l;
    }
    __syncthreads();
    // out: the piece's first and last word shared with its neighbours in the block
    uint32_t *dst = out + (gb >> 5);
    for (uint32_t i = tid; i < nw; i += ENC_TB) {
        if (i == 0 || i + 1 == nw) atomicOr(dst + i, s_img[i]);
        else dst[i] = s_img[i];
    }
}

// The items on the device, from the scan's arrays: what the host writes into
// its list from the blocks' bits (encode_blocks below), a thread per block.
__global__ __launch_bounds__(ENC_SCAN_TB) void k_encb_items(const uint64_t *__restrict__ bbits,
                                                            const uint64_t *__restrict__ wb, uint64_t nb, uint64_t n,
                                                            uint64_t block_syms, hh_batch_item *__restrict__ items) {
    const uint64_t b = (uint64_t)blockIdx.x * ENC_SCAN_TB + threadIdx.x;
    if (b >= nb) return;
    items[b] = hh_batch_item{4u * wb[b], bbits[b], b * block_syms, b + 1 < nb ? block_syms : n - b * block_syms};
}

// hh_encoder_encode_blocks (items on the host) and hh_encoder_encode_blocks_items
// (d_items on the device too; items may then be NULL).  The blocks' bits stay
// in enc->host_bits.
static int encode_blocks(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n, uint64_t block_syms,
                         void *d_out, uint64_t cap, hh_batch_item *d_items, bool to_device, hh_batch_item *items,
                         uint64_t *total_bytes, void *hip_stream) {
    if (!enc || !tree || !total_bytes || block_syms == 0 || (!d_out && cap)) return HH_ERR_ARG;
    if (n && (!d_syms || (to_device ? !d_items : !items))) return HH_ERR_ARG;
    if (((uintptr_t)d_items & 7u) != 0) return HH_ERR_ARG;  // (64-bit stores)
    if (((uintptr_t)d_out & 3u) != 0) return HH_ERR_ARG;   // (32-bit word stores)
    *total_bytes = 0;
    EncTab h;
    uint8_t len8[256];
    int rc = hh_codebook(tree, h.code, len8);
    if (rc) return rc;
    for (int i = 0; i < 256; i++) h.len[i] = len8[i];
    if (n == 0) return HH_OK;
    const uint64_t nb = n / block_syms + (n % block_syms != 0);
    if (nb >> 32) return HH_ERR_UNSUPPORTED;
    // (one block: its length is what counts, block_syms may be anything above)
    const uint64_t bsz = block_syms < n ? block_syms : n;
    const uint64_t ppb = (bsz + ENC_CH - 1) / ENC_CH, npc = nb * ppb;   // (npc < n / ENC_CH + 2 nb: no overflow)
    // (a launch's grid may not exceed 2^32 - 1 threads: about 2^24 pieces)
    if (npc * ENC_TB > 0xffffffffull) return HH_ERR_UNSUPPORTED;
    if (hipSetDevice(enc->device) != hipSuccess) return HH_ERR_DEVICE;
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t o_s = (sizeof(EncTab) + 255) & ~(size_t)255, o_bb = o_s + (((npc + 1) * 8 + 255) & ~(size_t)255),
                 o_wb = o_bb + ((nb * 8 + 255) & ~(size_t)255), o_res = o_wb + ((nb * 8 + 255) & ~(size_t)255);
    if (enc->size < o_res + 64) {
        // (the previous call on this encoder has returned: its stream is done
        // with the old workspace, no device-wide wait)
        if (enc->ws) (void)hipFree(enc->ws);
        enc->ws = nullptr;
        enc->size = 0;
        if (hipMalloc(&enc->ws, o_res + 64) != hipSuccess) return HH_ERR_NOMEM;
        enc->size = o_res + 64;
    }
    if (enc->host_bits_n < nb) {
        if (enc->host_bits) (void)hipHostFree(enc->host_bits);
        enc->host_bits = nullptr;
        enc->host_bits_n = 0;
        if (hipHostMalloc(&enc->host_bits, nb * 8, hipHostMallocDefault) != hipSuccess) return HH_ERR_NOMEM;
        enc->host_bits_n = nb;
    }
    uint8_t *ws = enc->ws;
    EncTab *d_tab = (EncTab *)ws;
    uint64_t *d_S = (uint64_t *)(ws + o_s), *d_bb = (uint64_t *)(ws + o_bb), *d_wb = (uint64_t *)(ws + o_wb),
             *d_res = (uint64_t *)(ws + o_res);
    uint32_t *d_bad = (uint32_t *)(ws + o_res + 32);
    uint64_t hres[5] = {0, 0, 0, 0, 0};
    rc = HH_ERR_DEVICE;
    do {
        if (hipMemcpyAsync(d_tab, &h, sizeof(h), hipMemcpyHostToDevice, st) != hipSuccess) break;
        if (hipMemsetAsync(ws + o_res, 0, 64, st) != hipSuccess) break;
        hipLaunchKernelGGL(k_encb_len, dim3((unsigned)npc), dim3(ENC_TB), 0, st, (const uint8_t *)d_syms, n, bsz,
                           (uint32_t)ppb, d_tab, d_S, d_bad);
        if (hipGetLastError() != hipSuccess) break;
        hipLaunchKernelGGL(k_encb_scan, dim3(1), dim3(ENC_SCAN_TB), 0, st, d_S, npc, (uint32_t)ppb, nb, d_bb, d_wb,
                           d_res);
        if (hipGetLastError() != hipSuccess) break;
        if (to_device) {
            hipLaunchKernelGGL(k_encb_items, dim3((unsigned)((nb + ENC_SCAN_TB - 1) / ENC_SCAN_TB)), dim3(ENC_SCAN_TB),
                               0, st, d_bb, d_wb, nb, n, block_syms, d_items);
            if (hipGetLastError() != hipSuccess) break;
        }
        if (hipMemcpyAsync(enc->host_bits, d_bb, nb * 8, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        if (hipMemcpyAsync(hres, d_res, 40, hipMemcpyDeviceToHost, st) != hipSuccess) break;
        if (hipStreamSynchronize(st) != hipSuccess) break;
        if ((uint32_t)hres[4]) { rc = HH_ERR_ARG; break; }   // (a symbol absent from the tree)
        uint64_t off = 0, sum = 0;
        for (uint64_t b = 0; b < nb; b++) {
            const uint64_t bits = enc->host_bits[b];
            if (items) {
                items[b].data_off = off;
                items[b].bits = bits;
                items[b].out_off = b * block_syms;
                items[b].cap = b + 1 < nb ? block_syms : n - b * block_syms;
            }
            off += (bits + 31) / 32 * 4;
            sum += bits;
        }
        if (sum != hres[0] || off != hres[1] * 4) { rc = HH_ERR_INTERNAL; break; }
        *total_bytes = off;
        if (off > cap) { rc = HH_ERR_CAPACITY; break; }
        if (hipMemsetAsync(d_out, 0, off, st) != hipSuccess) break;
        hipLaunchKernelGGL(k_encb_pack, dim3((unsigned)npc), dim3(ENC_TB), ENC_IMG_WORDS * 4, st,
                           (const uint8_t *)d_syms, n, bsz, (uint32_t)ppb, d_tab, d_S, d_wb, (uint32_t *)d_out);
        if (hipGetLastError() != hipSuccess) break;
        if (hipStreamSynchronize(st) != hipSuccess) break;
        rc = HH_OK;
    } while (0);
    return rc;
}

extern "C" int hh_encoder_encode_blocks(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                                        uint64_t block_syms, void *d_out, uint64_t cap, hh_batch_item *items,
                                        uint64_t *total_bytes, void *hip_stream) {
    return encode_blocks(enc, tree, d_syms, n, block_syms, d_out, cap, nullptr, false, items, total_bytes, hip_stream);
}

extern "C" int hh_encoder_encode_blocks_items(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                                              uint64_t block_syms, void *d_out, uint64_t cap, hh_batch_item *d_items,
                                              hh_batch_item *items, uint64_t *total_bytes, void *hip_stream) {
    return encode_blocks(enc, tree, d_syms, n, block_syms, d_out, cap, d_items, true, items, total_bytes, hip_stream);
}

// Compress into blocks: one histogram of all n bytes and one tree for all the
// blocks, then the blocked encode above, whose length pass makes the capacity
// check before a byte is written; the blocks' bits must add up to the
// histogram's sum of count x code length (as hh_compress_device checks its
// one stream).
// The bound: the code is shared, so one block of rare symbols may cost more
// than 8 bits per symbol; but all the blocks together are the text under the
// Huffman code of its own counts, at most 8 n bits (hh_compress_bound's
// argument), and a block of bits[b] bits takes ceil(bits[b] / 32) * 4 <
// bits[b] / 8 + 4 bytes: less than n + 4 nb in all.
extern "C" uint64_t hh_compress_blocks_bound(uint64_t n, uint64_t block_syms) {
    if (block_syms == 0) return 0;
    return (n + 3) / 4 * 4 + 4 * (n / block_syms + (n % block_syms != 0));
}

static int compress_blocks(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t block_syms, void *d_out,
                           uint64_t cap, hh_tree_buf *tree, hh_batch_item *d_items, bool to_device,
                           hh_batch_item *items, uint64_t *total_bytes, void *hip_stream) {
    if (!enc || !d_syms || !tree || (to_device ? !d_items : !items) || !total_bytes || n == 0 || block_syms == 0 ||
        (!d_out && cap))
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
    uint64_t pred = 0;
    for (int s = 0; s < 256; s++) pred += counts[s] * len8[s];   // (<= 64 n < 2^43)
    rc = encode_blocks(enc, &t, d_syms, n, block_syms, d_out, cap, d_items, to_device, items, total_bytes, hip_stream);
    if (rc != HH_OK && rc != HH_ERR_CAPACITY) return rc;
    const uint64_t nb = n / block_syms + (n % block_syms != 0);
    uint64_t got = 0;
    for (uint64_t b = 0; b < nb; b++) got += enc->host_bits[b];   // (the items' bits)
    if (got != pred) return HH_ERR_INTERNAL;
    return rc;
}

extern "C" int hh_compress_blocks_device(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t block_syms,
                                         void *d_out, uint64_t cap, hh_tree_buf *tree, hh_batch_item *items,
                                         uint64_t *total_bytes, void *hip_stream) {
    return compress_blocks(enc, d_syms, n, block_syms, d_out, cap, tree, nullptr, false, items, total_bytes,
                           hip_stream);
}

extern "C" int hh_compress_blocks_device_items(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t block_syms,
                                               void *d_out, uint64_t cap, hh_tree_buf *tree, hh_batch_item *d_items,
                                               hh_batch_item *items, uint64_t *total_bytes, void *hip_stream) {
    return compress_blocks(enc, d_syms, n, block_syms, d_out, cap, tree, d_items, true, items, total_bytes,
                           hip_stream);
}
