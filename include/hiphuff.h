/*
 * hiphuff.h -- C ABI of the MI355X-native parallel Huffman decoder.
 *
 * Plain C types only (pointers, sizes, status codes): this is the drop-in
 * boundary a host program links against (libhiphuff.so).  Each entry point
 * names the reference interface it replaces (BeauJoh/HuffmanDecoderOnGPUs,
 * paths relative to framework/).
 *
 * Layering
 *   hh_huff_*      .huff container (HUFF + 64-bit HUFX)     replaces huffdata.c:27-68
 *   hh_encode*, hh_tree_build, hh_histogram_device, hh_compress_device
 *                  the way back: bytes to a code and a stream (the reference
 *                  ships none)
 *   hh_decoder_*   device decoder state (tables, workspace)  replaces the lazy CL/CUDA
 *                                                             globals, openclapproach.c:231-234
 *   hh_decode_*    the hot path                               replaces openclApproach
 *                                                             (openclapproach.c:236-1047) and
 *                                                             fastgpuApproach (fastgpu.cu:140-332)
 *   hh_decode_batch_*  many streams of one code per launch   (the reference decodes one
 *                                                             stream per call)
 *   hh_encode_blocks*, hh_encoder_encode_blocks, hh_compress_blocks_*
 *                  the batch's producer: blocks of one text, each its own stream
 *   hh_encode_ragged*, hh_encoder_encode_ragged, hh_compress_ragged_*
 *                  the same for records of any lengths, cut at an offsets list
 *   hh_stage_*   reference-shaped stage kernels             replaces the six kernels of
 *                                                             ReleaseCL/kernels/ *.cl one by one
 *   hipHuffApproach  plugin with the reference's decoder       decodeUtil.h:14-19 function-pointer
 *                    signature (see hiphuff_plugin.h)          type, registered like mainrun.c:480-488
 *
 * Every function returns HH_OK (0) or a negative hh_status; nothing aborts
 * the process (the plugin wrapper converts errors to the reference's
 * exit(1) behaviour, decodeUtil.c:47-52).
 */
#ifndef HIPHUFF_H_
#define HIPHUFF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPHUFF_VERSION_MAJOR 0
#define HIPHUFF_VERSION_MINOR 1

typedef enum {
    HH_OK = 0,
    HH_ERR_ARG = -1,          /* bad argument (null pointer, size)            */
    HH_ERR_IO = -2,           /* file could not be opened / read / written    */
    HH_ERR_FORMAT = -3,       /* not a HUFF/HUFX container, truncated         */
    HH_ERR_TREE = -4,         /* tree is not a proper binary tree from node 0,
                                 or the root is a leaf (the reference loops
                                 forever on such a tree, pes.c:151-161)       */
    HH_ERR_CAPACITY = -5,     /* output buffer too small for the decode       */
    HH_ERR_DEVICE = -6,       /* HIP runtime error                            */
    HH_ERR_NOMEM = -7,        /* host or device allocation failed             */
    HH_ERR_INTERNAL = -8,     /* internal consistency check failed            */
    HH_ERR_TIMEOUT = -9,      /* bounded in-kernel wait expired               */
    HH_ERR_UNSUPPORTED = -10  /* input outside what this entry point handles  */
} hh_status;

const char *hh_strerror(int status);

/* ---------------------------------------------------------------------- */
/* Code tree.  Same information as struct HuffNode (huffdata.h:12-16):    */
/* node 0 is the root, a leaf has izero == ione == -1, bit 0 follows      */
/* izero, bit 1 follows ione.  Structure-of-arrays, no padding games.     */
/* ---------------------------------------------------------------------- */
typedef struct {
    int32_t nodes;
    const int32_t *izero;
    const int32_t *ione;
    const uint8_t *sym;
} hh_tree;

/* Static facts about a tree (validated: reachable part is a full binary
 * tree rooted at 0, no cycles). */
typedef struct {
    int32_t reachable;   /* nodes reachable from the root                 */
    int32_t leaves;      /* reachable leaves                              */
    int32_t minlen;      /* shortest code (tableMinDepth, huffdata.c:272) */
    int32_t maxlen;      /* longest code  (tableHeight,  huffdata.c:224)  */
    int32_t len_gcd;     /* gcd of all code lengths                       */
} hh_tree_info;

int hh_tree_check(const hh_tree *tree, hh_tree_info *info);

/* ---------------------------------------------------------------------- */
/* Container: loadHuffFile (huffdata.c:27-68) with 64-bit sizes.          */
/*   "HUFF": be-i32 nodes, be-i32 bits, be-i32 uncompressedsize,          */
/*           nodes x {u8 sym, be-i32 izero, be-i32 ione}, ceil(bits/8) B  */
/*   "HUFX": be-i32 nodes, be-i64 bits, be-i64 uncompressedsize, then the */
/*           same tree and payload (the 64-bit sibling for > 2^31 bits).  */
/* The loaded payload is followed by HH_PAYLOAD_PAD zero bytes.           */
/* ---------------------------------------------------------------------- */
#define HH_PAYLOAD_PAD 64

typedef struct {
    int32_t nodes;
    int32_t *izero;
    int32_t *ione;
    uint8_t *sym;
    uint64_t bits;
    uint64_t uncompressedsize;
    uint8_t *data;           /* ceil(bits/8) + HH_PAYLOAD_PAD bytes       */
    int wide;                /* 1 if read from / to be written as HUFX    */
} hh_huff;

int hh_huff_load(const char *path, hh_huff *out);
/* Writes HUFF when bits and size fit int32 (and !h->wide), else HUFX.    */
int hh_huff_save(const char *path, const hh_huff *h);
void hh_huff_free(hh_huff *h);
hh_tree hh_huff_tree(const hh_huff *h);

/* ---------------------------------------------------------------------- */
/* Encoder (the reference ships none).  Builds the    */
/* canonical bit strings of `tree` and packs `n` symbols LSB-first.       */
/* out must hold hh_encode_bound(tree, n) bytes; *bits gets the length.   */
/* Symbols absent from the tree are an HH_ERR_ARG.                        */
/* ---------------------------------------------------------------------- */
uint64_t hh_encode_bound(const hh_tree *tree, uint64_t n);
int hh_encode(const hh_tree *tree, const uint8_t *syms, uint64_t n,
              uint8_t *out, uint64_t *bits);
/* The same on the GPU through an encoder (its device's workspace, kept
 * across calls): n symbols at device pointer d_syms packed into device
 * buffer d_out (cap bytes, 4-byte aligned; it must hold the stream rounded
 * up to whole 32-bit words -- hh_encode_bound always does).  The same bytes
 * as hh_encode.  *bits gets the length (also with HH_ERR_CAPACITY).
 * Enqueued on hip_stream; returns when done.  One call at a time per
 * encoder; encoders are independent (one per stream encodes at once).  At
 * most about 2^36 symbols per call (HH_ERR_UNSUPPORTED beyond: the launch's
 * grid limit). */
typedef struct hh_encoder hh_encoder;
int hh_encoder_create(hh_encoder **enc, int device);
void hh_encoder_destroy(hh_encoder *enc);
int hh_encoder_encode(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                      void *d_out, uint64_t cap, uint64_t *bits, void *hip_stream);
/* hh_encoder_encode on a process-wide encoder of the current device (calls
 * serialised on it). */
int hh_encode_device(const hh_tree *tree, const void *d_syms, uint64_t n,
                     void *d_out, uint64_t cap, uint64_t *bits, void *hip_stream);

/* ---------------------------------------------------------------------- */
/* Compression: from bytes to a code and a stream (the reference ships    */
/* .huff files and no way to make one).                                   */
/* ---------------------------------------------------------------------- */
/* Huffman tree of byte counts, on the host.  Deterministic: the live items
 * are the symbols with counts[s] > 0 (k of them); the two smallest keys
 * (count, order) a then b are merged into a node of count a + b with
 * zero-child a and one-child b, where a leaf's order is its symbol value and
 * the i-th node created has order k + i (a leaf before a node of the same
 * count and order).  Laid out in pre-order (node 0 the root, then the zero
 * subtree, then the one subtree; internal nodes sym 0).  One distinct symbol
 * s: three nodes, leaf s on the zero side and leaf (s + 1) & 255 on the one
 * side (a root leaf is no tree, HH_ERR_TREE above).  HH_ERR_ARG: all counts
 * zero, or their total overflows uint64_t.  No limit on the code length
 * here; the encoders answer HH_ERR_UNSUPPORTED for codes over 64 bits
 * (a code of depth d needs a total of about Fib(d + 1): the 2^36 symbols an
 * encoder call takes cannot give one). */
#define HH_BUILD_MAX_NODES 511
typedef struct {
    int32_t nodes;
    int32_t izero[HH_BUILD_MAX_NODES];
    int32_t ione[HH_BUILD_MAX_NODES];
    uint8_t sym[HH_BUILD_MAX_NODES];
} hh_tree_buf;
int hh_tree_build(const uint64_t counts[256], hh_tree_buf *out);

/* Exact counts of the n bytes at device pointer d_syms (any alignment) into
 * counts[256] on the host.  Enqueued on hip_stream; returns when done.  The
 * scratch is the encoder's (one call at a time per encoder).  n == 0: all
 * zero.  At most about 2^36 bytes, as hh_encoder_encode. */
int hh_histogram_device(hh_encoder *enc, const void *d_syms, uint64_t n,
                        uint64_t counts[256], void *hip_stream);

/* Histogram, hh_tree_build, hh_encoder_encode in one call: n > 0 bytes at
 * d_syms compressed into d_out (cap bytes, 4-byte aligned) with their own
 * Huffman code, which *tree receives; *bits the stream's length.
 * hh_compress_bound(n) = n rounded up to 4 bytes always suffices (a Huffman
 * code over bytes never exceeds 8 bits per symbol on average, and the encoder
 * writes whole 32-bit words).  HH_ERR_CAPACITY is found before any encode
 * kernel runs, *tree and *bits filled.  Add HH_PAYLOAD_PAD bytes to decode
 * d_out in place. */
uint64_t hh_compress_bound(uint64_t n);
int hh_compress_device(hh_encoder *enc, const void *d_syms, uint64_t n,
                       void *d_out, uint64_t cap, hh_tree_buf *tree,
                       uint64_t *bits, void *hip_stream);

/* ---------------------------------------------------------------------- */
/* Device decoder.                                                        */
/* ---------------------------------------------------------------------- */
typedef struct hh_decoder hh_decoder;

typedef struct {
    int device;              /* HIP device ordinal                           */
    int lane_bits;           /* bits per lane region, 0 = default            */
    int flags;               /* HH_FLAG_*                                    */
} hh_config;

#define HH_FLAG_FORCE_EXACT 1   /* skip the fast path and decode with the
                                   reference-shaped stage pipeline (the six
                                   hh_stage_* kernels: exact, O(25 * bits)
                                   memory, bits < 2^31) */
#define HH_FLAG_FORCE_SEGMENT 2 /* skip the fast path and decode with the
                                   segment path (exact, O(N), any length;
                                   the path codes that do not resynchronise
                                   take, codes <= 32 bits) */
#define HH_FLAG_NO_FIXED 4      /* a complete fixed-length code (2^L symbols,
                                   every code L <= 8 bits, e.g. E.coli's) is
                                   unpacked directly (k_fixed) unless this is
                                   set: then it takes the general pipeline */
#define HH_FLAG_LEGACY 8        /* decode with round 2's pipeline (k_front,
                                   k_walk, k_table, k_scan, k_emit) instead of
                                   the state-machine decode (k_cnt, k_fscan,
                                   k_emf) */
#define HH_FLAG_PHASE_TIMING 16 /* record a HIP event between the count, scan
                                   and emission kernels of every decode, for
                                   ms_sync / ms_scan / ms_emit (each event
                                   adds ~6 us of idle GPU time between the
                                   kernels it separates; without the flag
                                   only ms_total is measured, the phase times
                                   read 0) */
#define HH_FLAG_KEEP_HOST_PINNED 32 /* hh_decode_host keeps the caller's payload
                                   and output buffers page-locked across calls
                                   (hipHostRegister once per buffer: a call
                                   with another pointer or a longer length
                                   re-registers) instead of registering and
                                   releasing them in every call.  The caller
                                   must not free or unmap a buffer the decoder
                                   holds: release it first with
                                   hh_decoder_release_host (hh_decoder_destroy
                                   releases them too).  For a harness that
                                   decodes the same buffers again and again,
                                   as the reference's evaluate() does
                                   (decodeUtil.c:41-43, 54-68). */
#define HH_FLAG_TWO_PASS 64     /* the state-machine decode in its two-pass
                                   form (k_cntm count pass, k_fscan1 scan,
                                   k_emf emission) instead of the single pass
                                   (k_one: speculative emission, decoupled
                                   look-back); HH_FLAG_PHASE_TIMING implies
                                   it (the split is between its kernels) */

int hh_decoder_create(hh_decoder **dec, const hh_config *cfg);
void hh_decoder_destroy(hh_decoder *dec);

/* Upload / replace the code tree (builds the lookup tables on the host,
 * copies them to the device).  The tree may be reused across decodes. */
int hh_decoder_set_tree(hh_decoder *dec, const hh_tree *tree);

/* Statistics of the last decode (device time of each phase, in ms). */
typedef struct {
    double ms_total;         /* hipEvent time of the whole device pipeline  */
    double ms_sync;          /* count kernels: heads, region counts, walks
                                (state machine: HH_FLAG_PHASE_TIMING only)  */
    double ms_scan;          /* scan kernels: tile bases, total (idem)      */
    double ms_emit;          /* emission kernels: symbols to HBM (idem)     */
    uint64_t out_len;        /* symbols decoded                              */
    uint64_t lanes;          /* lane regions                                 */
    uint64_t repairs;        /* 1: a tile-state chain was composed on the
                                host (or the stage pipeline ran)            */
    int exact_fallback;      /* 0: the fast path decoded; 1: the stage
                                pipeline (codes longer than 32 bits); 2: the
                                segment path (a walk found no merge: a code
                                that does not resynchronise)                */
    int fixed_length;        /* 1: a complete fixed-length code, unpacked
                                by k_fixed (HH_FLAG_NO_FIXED: 0)            */
    int state_machine;       /* the state-machine decode ran: 1 its two
                                passes (k_cntm, k_fscan1, k_emf), 2 its
                                single pass (k_one), 3 the batched decode
                                (k_batch, hh_decode_batch_device)           */
} hh_stats;

int hh_decoder_stats(const hh_decoder *dec, hh_stats *st);

/* Decode `bits` bits at device pointer d_data (it must be readable for
 * ceil(bits/8) + HH_PAYLOAD_PAD bytes; the pad content is ignored) into
 * device buffer d_out (cap bytes).  *out_len receives the number of
 * symbols, i.e. the length the reference computes with findmax + 1
 * (findmax.cl:2-8).  Enqueued on `hip_stream` (a hipStream_t, NULL = the
 * default stream); the call returns after the output length is known.
 * HH_ERR_CAPACITY (the decode needs more than cap bytes): *out_len is still
 * the stream's full symbol count -- the size to retry with -- here and in
 * hh_decode_host; the output buffer's content is then unspecified.  On
 * HH_ERR_CAPACITY, as on success, nothing at or beyond d_out + cap is
 * written.                                                                */
int hh_decode_device(hh_decoder *dec, const void *d_data, uint64_t bits,
                     void *d_out, uint64_t cap, uint64_t *out_len,
                     void *hip_stream);

/* Asynchronous form of hh_decode_device for a stream of decodes: enqueues
 * the decode on `hip_stream` and returns before it has run, then checks the
 * decode issued before it (its length into the out_len pointer passed with
 * it), so that the GPU has the next decode queued while the host reads the
 * last one's results instead of idling between synchronous calls.
 * hh_decode_wait checks the last one and returns the first failure of the
 * asynchronous decodes since the previous wait (HH_OK if none), as
 * hh_decode_device would have returned it; a stream that does not
 * resynchronise is decoded again on the exact path there.  Every out_len
 * pointer and output buffer must stay valid until hh_decode_wait returns.
 * The call itself returns HH_OK, or the argument / launch failure of this
 * decode.  Paths other than the state machine and k_fixed decode
 * synchronously inside the call.  Other entry points (hh_decode_device,
 * ranges, host decodes) first check a pending asynchronous decode.
 * Consecutive asynchronous decodes may use different streams: the decoder's
 * workspace is shared, so a decode on another stream than the pending one
 * is ordered after that one's last kernel (hipStreamWaitEvent). */
int hh_decode_device_async(hh_decoder *dec, const void *d_data, uint64_t bits,
                           void *d_out, uint64_t cap, uint64_t *out_len,
                           void *hip_stream);
int hh_decode_wait(hh_decoder *dec);

/* ---------------------------------------------------------------------- */
/* Batched decode: n independent streams of the decoder's code in ONE     */
/* kernel launch (k_batch), for many small blocks coded with one shared   */
/* code -- chunked files, records, pages -- where a call per stream costs */
/* its launches' fixed time n times over.                                 */
/* ---------------------------------------------------------------------- */
typedef struct {
    uint64_t data_off;   /* byte offset of the stream's payload in d_data; a multiple of 4 */
    uint64_t bits;       /* stream length; 0 is allowed (out_len 0, nothing written)        */
    uint64_t out_off;    /* byte offset of its output in d_out; any alignment              */
    uint64_t cap;        /* bytes it may write at out_off                                  */
} hh_batch_item;

/* Stream i decodes exactly as hh_decode_device(dec, d_data + data_off, bits,
 * d_out + out_off, cap, ...) would on its own: the same bytes, the same
 * out_len[i] (findmax + 1, the tail rule included), each stream from the
 * root.  Capacity is per stream: status[i] = HH_ERR_CAPACITY, out_len[i] the
 * stream's full symbol count, nothing written at or beyond out_off + cap;
 * one stream's failure does not disturb the others.  Returns HH_OK if every
 * stream is HH_OK, else the status of the lowest-index failing stream
 * (status may be NULL).  items, out_len and status are host arrays of n.
 * HH_ERR_ARG, before any launch and with nothing written: a data_off that is
 * no multiple of 4 (or d_data off a 4-byte boundary); for bits > 0,
 * data_off + ceil(bits/8) + HH_PAYLOAD_PAD > data_bytes; out_off + cap >
 * out_bytes; no tree set; a null pointer with n > 0.  n == 0 returns HH_OK.
 * Payloads may overlap or lie back to back at 4-byte boundaries: the next
 * stream's bytes serve as the readable pad (pad content is ignored).
 * Output ranges must not overlap -- the caller's duty, not checked; they
 * may touch at any alignment (a stream's first and last bytes are stored as
 * bytes, never as part of a wider store that covers a neighbour's).
 * Trees: every tree the decoder holds state-machine tables for -- at most
 * 255 internal nodes, any byte-alphabet code, whatever HH_FLAG_* the decoder
 * was created with -- whose emission tables leave room in the LDS for one
 * tile's payload and staging (every tree at the default settings); other
 * trees return HH_ERR_UNSUPPORTED.  Fixed-length codes, codes longer than 32
 * bits and codes that do not resynchronise decode exactly here itself (the
 * last slowly: a region per fix round); there is no fallback path.  n < 2^32.
 * A stream is decoded by one workgroup, round by round: a very large stream
 * is hh_decode_device's work, which spreads it over the whole GPU.
 * Enqueued on hip_stream; returns when done.  A pending asynchronous decode
 * is checked first (its status kept for hh_decode_wait).  hh_stats after a
 * batch: out_len the sum over the streams, lanes the regions of all of
 * them, ms_total the launch's device time, state_machine 3. */
int hh_decode_batch_device(hh_decoder *dec, const void *d_data, uint64_t data_bytes,
                           const hh_batch_item *items /* host */, uint64_t n,
                           void *d_out, uint64_t out_bytes,
                           uint64_t *out_len /* host, n */, int32_t *status /* host, n, may be NULL */,
                           void *hip_stream);
/* The tiles (of hh_decoder_tile_bits() bits, 64 regions) a workgroup of the
 * batched decode takes per round for the current tree: where a stream's
 * length changes its number of rounds.  HH_ERR_UNSUPPORTED as above. */
int hh_decode_batch_round_tiles(const hh_decoder *dec, uint32_t *tiles);

/* What a batch of device items came to, for a caller that reads one record
 * instead of two arrays (hh_decode_batch_device_items writes it on the
 * device, in stream order, like the arrays). */
typedef struct {
    uint64_t total_len;      /* sum of out_len over the streams with status HH_OK or HH_ERR_CAPACITY */
    uint32_t n_failed;       /* streams whose status != HH_OK */
    uint32_t first_failed;   /* lowest such index (0xffffffff: none) */
    int32_t  first_status;   /* its status (HH_OK: none) */
    uint32_t pad;
} hh_batch_summary;

/* hh_decode_batch_device with everything per stream on the device and in
 * stream order: d_items, d_out_len and d_status are device arrays of n,
 * d_summary a device record (may be NULL; 8-byte aligned).  Stream i gives
 * the bytes, d_out_len[i] and d_status[i] that hh_decode_batch_device gives
 * for the same item -- per-stream capacity, bits == 0, outputs that touch at
 * any alignment, the same trees (HH_ERR_UNSUPPORTED otherwise), n < 2^32 - 1.
 * Stream ordered: everything is enqueued on hip_stream and the call returns
 * without waiting for the device.  d_items and d_data are read in the order
 * of hip_stream (work queued before the call on that stream may still be
 * producing them); d_out, d_out_len, d_status and d_summary are complete when
 * the stream reaches the end of the call's work.  The call issues no stream,
 * device or event synchronisation and no device-to-host copy, and puts
 * nothing on the null stream -- with one exception: a call that must grow
 * the decoder's batch workspace waits for the previous batch's end before it
 * frees the old one; a call that finds the workspace large enough never
 * blocks.  d_items must stay valid until the stream has passed the call's
 * first kernel (the only one that reads it); d_data and the result arrays
 * until the end of the call's work.
 * Checked on the host, before anything is enqueued: HH_ERR_ARG for a null
 * pointer with n > 0 (d_summary excepted), d_data off a 4-byte boundary, no
 * tree set; HH_ERR_UNSUPPORTED for a tree the batch cannot take or n >= 2^32
 * - 1.  n == 0 returns HH_OK and enqueues nothing, except that a d_summary
 * given is set to the empty summary {0, 0, 0xffffffff, HH_OK} (memsets on
 * hip_stream).
 * Checked on the device, per item (the host never sees the items): the
 * three rules of hh_decode_batch_device -- data_off a multiple of 4; for
 * bits > 0, data_off + ceil(bits/8) + HH_PAYLOAD_PAD <= data_bytes; out_off
 * + cap <= out_bytes, none of the sums overflowing.  An item that breaks one
 * gets d_status[i] = HH_ERR_ARG and d_out_len[i] = 0; not a byte is read or
 * written for it, and the other streams decode normally.  (The one
 * deliberate difference from hh_decode_batch_device, which rejects the whole
 * batch.)  A slot the decode kernel did not reach reports HH_ERR_INTERNAL.
 * The return value says what was enqueued, never how the streams fared:
 * that is in d_status and d_summary.
 * With the decoder's other calls: the decoder records an event after the
 * batch's last kernel.  hh_decoder_set_tree and hh_decoder_destroy wait for
 * it on the host; hh_decode_batch_device and an hh_decode_batch_device_items
 * on another stream make their stream wait for it (the batch workspace is
 * one per decoder); a later items batch on the same stream is ordered by the
 * stream.  The single-stream decodes do not share that workspace and need no
 * wait; a pending hh_decode_device_async is not checked by this call and
 * stays pending.  hh_stats after the call: all zero but state_machine = 3
 * (the host knows no lengths). */
int hh_decode_batch_device_items(hh_decoder *dec, const void *d_data, uint64_t data_bytes,
                                 const hh_batch_item *d_items /* device, n */, uint64_t n,
                                 void *d_out, uint64_t out_bytes,
                                 uint64_t *d_out_len /* device, n */, int32_t *d_status /* device, n */,
                                 hh_batch_summary *d_summary /* device, may be NULL */,
                                 void *hip_stream);

/* Random access into a block-coded buffer: byte ranges of the uncompressed
 * data, each delivered to a destination of its own, in one stream-ordered
 * call. */
typedef struct {
    uint64_t src_off;   /* first byte of the range in the uncompressed data */
    uint64_t len;       /* bytes; 0 is allowed                               */
    uint64_t dst_off;   /* where the bytes go in d_out; any alignment        */
} hh_block_read;

/* The blocked buffer is what hh_encoder_encode_blocks_items (or
 * hh_compress_blocks_device_items) leaves behind: n_syms symbols in nb =
 * ceil(n_syms / block_syms) blocks, block b the symbols [b * block_syms,
 * min(n_syms, (b + 1) * block_syms)), d_index[b] its item.  Of d_index[b]
 * only data_off and bits are read; out_off and cap are ignored (the block's
 * place and size follow from n_syms and block_syms).
 * Read i delivers the bytes [src_off, src_off + len) of the uncompressed
 * data to d_out + dst_off: the same bytes as that slice of a full decode.  A
 * read may cross any number of block edges.  Of each touched block only the
 * rounds up to the one that holds the read's last byte are walked; nothing
 * is decoded into a scratch buffer.  Destination ranges of different reads
 * must not overlap -- the caller's duty, as for hh_decode_batch_device; they
 * may touch at any alignment (no byte a read does not own is stored, and no
 * wider store covers a neighbour's byte).
 * Stream ordered, exactly as hh_decode_batch_device_items: everything is
 * enqueued on hip_stream; no synchronisation, no device-to-host copy,
 * nothing on the null stream (but for the wait before the batch workspace
 * grows, as there); d_reads and d_index are read in stream order by the
 * plan's kernels only; d_out, d_read_len, d_status and d_summary are
 * complete when the stream has passed the call's work.  The call shares the
 * decoder's batch workspace and its end event: hh_decoder_set_tree,
 * hh_decoder_destroy, hh_decode_batch_device and a batch on another stream
 * behave towards it as towards an items batch.  hh_stats after the call: all
 * zero but state_machine = 3.
 * Checked on the host, before anything is enqueued: HH_ERR_ARG for a null
 * pointer with m > 0 (d_summary excepted; d_index only when n_syms > 0),
 * block_syms == 0, d_data off a 4-byte boundary, no tree set;
 * HH_ERR_UNSUPPORTED for a tree the batch cannot take, or a piece budget
 * P = out_bytes / block_syms + 2 m of 2^32 - 1 or more (reads with disjoint
 * destinations never have more pieces than P; the workspace is sized by it:
 * 133 P + 52 m bytes and some).  m == 0 returns HH_OK, sets a d_summary
 * given to the empty summary and enqueues nothing else.
 * Checked on the device, per read, overflow-safe: src_off + len <= n_syms,
 * dst_off + len <= out_bytes; for every block the read touches, the index
 * entry's payload rules (data_off a multiple of 4; for bits > 0, data_off +
 * ceil(bits/8) + HH_PAYLOAD_PAD <= data_bytes).
 * d_status[i]: HH_OK, d_read_len[i] == len.  HH_ERR_ARG: the read is out of
 * range (it gets no piece: not a byte is read or written for it, d_read_len
 * [i] = 0); or a touched index entry breaks a rule (that block's part is
 * neither read nor written, the read's other parts may be); or the reads'
 * pieces exceed P (overlapping destinations only).  HH_ERR_FORMAT: a block's
 * stream ended before its part of the read was filled -- index and data
 * disagree; d_read_len[i] is the number of bytes delivered.
 * HH_ERR_INTERNAL: as in the items call.  A failing read's status is that of
 * its lowest-numbered failing block.  In every case nothing outside
 * [dst_off, dst_off + len) is written and the other reads are undisturbed.
 * d_summary: total_len the delivered bytes of the HH_OK reads, n_failed,
 * first_failed, first_status over the reads. */
int hh_decode_blocks_read(hh_decoder *dec, const void *d_data, uint64_t data_bytes,
                          const hh_batch_item *d_index /* device, nb */,
                          uint64_t n_syms, uint64_t block_syms,
                          const hh_block_read *d_reads /* device, m */, uint64_t m,
                          void *d_out, uint64_t out_bytes,
                          uint64_t *d_read_len /* device, m */, int32_t *d_status /* device, m */,
                          hh_batch_summary *d_summary /* device, may be NULL */,
                          void *hip_stream);

/* The same reads with every touched block walked at most once per call,
 * however many reads fall into it: for dense small reads (records by row
 * id, pages of a column, a gather), where hh_decode_blocks_read decodes a
 * block from its root once per read that touches it.
 * Equal to hh_decode_blocks_read: the arguments and their meaning; for every
 * input the bytes in d_out, d_read_len, d_status and d_summary (statuses of
 * out-of-range and empty reads, bad index entries, blocks that end early and
 * the piece budget P included; the content of overlapping destinations is
 * unspecified in both calls); the host checks; the stream-order rules (no
 * synchronisation, no device-to-host copy, nothing on the null stream but
 * for the wait before the workspace grows); the shared batch workspace and
 * end event; hh_stats after the call.
 * Different: one more host check -- nb = ceil(n_syms / block_syms) of 2^32 -
 * 1 or more is HH_ERR_UNSUPPORTED, before any allocation -- because the call
 * keeps 20 bytes per block (its pieces' count, list position and cursor, the
 * end of its last window) and 32 per block that can be touched, min(nb, P),
 * beside hh_decode_blocks_read's 133 P + 52 m bytes; and every call does
 * O(nb) work to clear and scan those, whatever the reads.  Of a touched
 * block the rounds up to the one that holds the last byte any read wants of
 * it are walked, once; a round in which no read has a byte is counted and
 * not emitted.
 * Which to use (measured: DESIGN.md section 13): this call when several
 * reads may fall into one block; hh_decode_blocks_read when reads are sparse
 * (at most about one per touched block) or nb is far larger than the number
 * of reads, where the per-block bookkeeping buys nothing. */
int hh_decode_blocks_gather(hh_decoder *dec, const void *d_data, uint64_t data_bytes,
                            const hh_batch_item *d_index /* device, nb */,
                            uint64_t n_syms, uint64_t block_syms,
                            const hh_block_read *d_reads /* device, m */, uint64_t m,
                            void *d_out, uint64_t out_bytes,
                            uint64_t *d_read_len /* device, m */, int32_t *d_status /* device, m */,
                            hh_batch_summary *d_summary /* device, may be NULL */,
                            void *hip_stream);

/* Record take: the records of a coded column named by a list of ids, their
 * bytes one after another in d_out and the offsets that delimit them -- an
 * Arrow `take` on a string column, a gather of rows by id.  d_index is the
 * list hh_encoder_encode_ragged (or hh_encoder_encode_blocks_items: take by
 * block id) leaves on the device; of an entry only data_off, bits and cap --
 * the record's length in symbols -- are read, out_off is ignored.  d_ids: m
 * record ids (NULL: the records 0 .. nrec - 1 in order, m == nrec); ids may
 * repeat and come in any order.
 * For taken record j, r = d_ids[j]: len_j = d_index[r].cap when r < nrec and
 * the entry keeps the payload rules (data_off a multiple of 4; for bits > 0,
 * data_off + ceil(bits/8) + HH_PAYLOAD_PAD <= data_bytes, no sum
 * overflowing); else len_j = 0, d_status[j] = HH_ERR_ARG and the record
 * reads and writes nothing.  d_out_offs[j] = the sum of len_i over i < j,
 * d_out_offs[m] the total, saturating; all m + 1 are written whatever the
 * statuses (a caller whose buffer was too small reads the size it needs in
 * d_out_offs[m]).  A record with d_out_offs[j + 1] > out_bytes gets
 * HH_ERR_CAPACITY and is not decoded; those before it that fit decode.
 * Otherwise the record's stream is decoded from the root, exactly as
 * hh_decode_device decodes it alone (tail rule included), to d_out +
 * d_out_offs[j]: holding c symbols, HH_OK when c == len_j, else
 * HH_ERR_FORMAT (index and data disagree); in both cases exactly the first
 * min(c, len_j) symbols are delivered and the rest of the record's range is
 * untouched.  No byte is stored outside [d_out_offs[j], d_out_offs[j + 1])
 * for record j, none at or beyond d_out + out_bytes, and no wide store
 * covers a byte that is not the call's; d_out may have any alignment.  An
 * empty record (bits == 0, cap == 0) is HH_OK.
 * d_summary: total_len the sum of len_j over the HH_OK records; n_failed,
 * first_failed, first_status as in hh_decode_batch_device_items, whose empty
 * summary m == 0 gives (and enqueues nothing else).
 * Many records share a round of the decode kernel (64 x tiles lanes, a lane
 * per region of hh_decoder_tile_bits() / 64 bits: hh_decode_take_round_tiles),
 * so short records cost their bits, not a round each.
 * Stream order, the decoder's end event, the batch workspace (80 bytes per
 * taken record and some) and hh_stats: hh_decode_batch_device_items' rules,
 * word for word -- everything on hip_stream, no synchronisation, no
 * device-to-host copy, nothing on the null stream but where the workspace
 * must grow; d_ids and d_index are read by the call's first kernel only.
 * Host checks: HH_ERR_ARG for a null pointer with m > 0 (d_summary and d_ids
 * excepted; d_index only when nrec > 0), d_data off a 4-byte or d_out_offs
 * off an 8-byte boundary, no tree set, d_ids == NULL with m != nrec;
 * HH_ERR_UNSUPPORTED for a tree the batch cannot take, m or nrec >= 2^32 - 1. */
int hh_decode_batch_take(hh_decoder *dec, const void *d_data, uint64_t data_bytes,
                         const hh_batch_item *d_index /* device, nrec */, uint64_t nrec,
                         const uint64_t *d_ids /* device, m; NULL: records 0..nrec-1 in order, m == nrec */,
                         uint64_t m,
                         void *d_out, uint64_t out_bytes,
                         uint64_t *d_out_offs /* device, m + 1 */,
                         int32_t *d_status /* device, m */,
                         hh_batch_summary *d_summary /* device, may be NULL */,
                         void *hip_stream);
/* The tiles per round of the take's kernel for the current tree (its marks
 * take LDS the batched decode does not need: for some trees one tile fewer
 * than hh_decode_batch_round_tiles). */
int hh_decode_take_round_tiles(const hh_decoder *dec, uint32_t *tiles);

/* ---------------------------------------------------------------------- */
/* Blocked encode: the producer of a batch. n symbols are cut into       */
/* nb = ceil(n / block_syms) blocks, block b the symbols                  */
/* [b * block_syms, min(n, (b + 1) * block_syms)), and every block is     */
/* encoded on its own from the root, exactly as hh_encode would encode    */
/* those symbols alone -- all of them in one call (one set of launches).  */
/* ---------------------------------------------------------------------- */
/* Layout: block b starts at byte data_off[b] of the output, data_off[0] = 0,
 * data_off[b + 1] = data_off[b] + ceil(bits[b] / 32) * 4 (every block starts
 * on a 4-byte boundary), *total_bytes = data_off[nb]; the bits between a
 * block's last bit and the next 4-byte boundary are zero.  items (host, nb
 * entries) receives items[b] = {data_off[b], bits[b], out_off = b *
 * block_syms, cap = the symbols in block b}: the array passes unchanged to
 * hh_decode_batch_device, which gives the symbols back in place.  For that
 * decode the caller allocates *total_bytes + HH_PAYLOAD_PAD bytes for d_out
 * (the last block's readable pad; its content is ignored).
 * hh_encode_blocks_bound: bytes that always hold the blocked stream of n
 * symbols of tree -- per block ceil(len_b * maxlen / 8) rounded up to 4,
 * summed; 0 for a bad tree (as hh_encode_bound) or block_syms == 0.
 * hh_encode_blocks: the host reference, the same bytes and items as the
 * device call (out: cap bytes, any alignment).
 * hh_encoder_encode_blocks: on the GPU through an encoder (its workspace,
 * grown on demand), d_syms and d_out device pointers, d_out 4-byte aligned.
 * Enqueued on hip_stream, returns when done, as hh_encoder_encode; one call
 * at a time per encoder; no device-wide wait, nothing on the null stream.
 * Nothing is written at or beyond d_out + *total_bytes.
 * HH_ERR_ARG: block_syms == 0, a null pointer with n > 0, d_out off a 4-byte
 * boundary, a symbol absent from the tree in any block.  HH_ERR_CAPACITY:
 * *total_bytes > cap, found after the length pass and before any byte of the
 * output is written; items and *total_bytes are filled (the size to retry
 * with).  HH_ERR_UNSUPPORTED (device call): nb >= 2^32, more pieces than a
 * launch's grid holds (nb * ceil(block_syms / 4096) above about 2^24), codes
 * over 64 bits.  n == 0: HH_OK, *total_bytes = 0, nothing written. */
uint64_t hh_encode_blocks_bound(const hh_tree *tree, uint64_t n, uint64_t block_syms);
int hh_encode_blocks(const hh_tree *tree, const uint8_t *syms, uint64_t n, uint64_t block_syms,
                     uint8_t *out, uint64_t cap, hh_batch_item *items, uint64_t *total_bytes);
int hh_encoder_encode_blocks(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                             uint64_t block_syms, void *d_out, uint64_t cap,
                             hh_batch_item *items /* host, nb */, uint64_t *total_bytes,
                             void *hip_stream);
/* hh_encoder_encode_blocks that also leaves the items on the device: d_items
 * (device, nb entries, 8-byte aligned; required when n > 0) receives the same
 * items[b], written by a kernel from the block scan's arrays, and goes
 * straight into hh_decode_batch_device_items with no upload.  items (host)
 * may be NULL.  Everything else -- synchronous, the capacity rule, the
 * errors, what HH_ERR_CAPACITY leaves filled (d_items too) -- as
 * hh_encoder_encode_blocks. */
int hh_encoder_encode_blocks_items(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                                   uint64_t block_syms, void *d_out, uint64_t cap,
                                   hh_batch_item *d_items /* device, nb */,
                                   hh_batch_item *items /* host, nb, may be NULL */,
                                   uint64_t *total_bytes, void *hip_stream);
/* Compress into blocks: the histogram of all n > 0 bytes, hh_tree_build, then
 * hh_encoder_encode_blocks with that one tree, which *tree receives (also
 * with HH_ERR_CAPACITY).  The blocks' bits must add up to the histogram's
 * sum of count x code length, else HH_ERR_INTERNAL.  n == 0: HH_ERR_ARG, as
 * hh_compress_device.
 * hh_compress_blocks_bound(n, block_syms) = (n + 3) / 4 * 4 + 4 * nb always
 * suffices: the code is shared by all blocks, so a single block of rare
 * symbols may cost more than 8 bits per symbol, but the total is at most 8 n
 * bits (hh_compress_bound's argument: a Huffman code over bytes never exceeds
 * 8 bits per symbol on average over its own text), and rounding a block up to
 * a whole 32-bit word adds less than 4 bytes per block.  0 for block_syms ==
 * 0.  Add HH_PAYLOAD_PAD bytes to decode d_out in place. */
uint64_t hh_compress_blocks_bound(uint64_t n, uint64_t block_syms);
int hh_compress_blocks_device(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t block_syms,
                              void *d_out, uint64_t cap, hh_tree_buf *tree,
                              hh_batch_item *items /* host, nb */, uint64_t *total_bytes,
                              void *hip_stream);
/* The same chain with hh_encoder_encode_blocks_items at its end: d_items
 * (device, nb) is filled, items (host) may be NULL. */
int hh_compress_blocks_device_items(hh_encoder *enc, const void *d_syms, uint64_t n, uint64_t block_syms,
                                    void *d_out, uint64_t cap, hh_tree_buf *tree,
                                    hh_batch_item *d_items /* device, nb */,
                                    hh_batch_item *items /* host, nb, may be NULL */,
                                    uint64_t *total_bytes, void *hip_stream);

/* ---------------------------------------------------------------------- */
/* Ragged blocked encode: records of any lengths.  n symbols are cut at   */
/* a list of offsets: offs has nrec + 1 values, offs[0] == 0,             */
/* nondecreasing, offs[nrec] == n; record r is the symbols                 */
/* [offs[r], offs[r + 1]) and may be empty.  Every record is encoded on   */
/* its own from the root, exactly as hh_encode would encode those symbols */
/* alone -- all of them in one call.                                       */
/* ---------------------------------------------------------------------- */
/* Layout: the blocks' (above) with records for blocks.  Record r starts at
 * byte data_off[r], data_off[0] = 0, data_off[r + 1] = data_off[r] +
 * ceil(bits[r] / 32) * 4; the bits between a record's end and the next
 * 4-byte boundary are zero; an empty record has bits 0, takes no bytes and
 * shares its data_off with its successor.  *total_bytes = data_off[nrec];
 * nothing is written at or beyond it.  items[r] = {data_off[r], bits[r],
 * out_off = offs[r], cap = offs[r + 1] - offs[r]}: the list goes unchanged
 * into hh_decode_batch_device(_items), which gives the text back in place
 * (any subset of its rows gives those records).  With offs[r] = min(n, r * B)
 * the bytes, the items and the total are hh_encode_blocks' for block_syms = B.
 * hh_encode_ragged_bound: bytes that hold the ragged stream of any valid
 * offs: ceil(n * maxlen / 8) + 4 * nrec, rounded up to 4; 0 for a bad tree.
 * hh_encode_ragged: the host reference (syms, offs, out, items on the host;
 * out any alignment; items may be NULL).
 * hh_encoder_encode_ragged: on the GPU through an encoder (its workspace,
 * grown on demand).  d_syms, d_offs (nrec + 1 values, 8-byte aligned) and
 * d_out (4-byte aligned) are device pointers; d_items (device, nrec entries,
 * 8-byte aligned, may be NULL) and items (host, nrec entries, may be NULL)
 * receive the list.  With items == NULL nothing per record crosses to the
 * host: only the totals and the flags come back.  Enqueued on hip_stream,
 * returns when done, one call at a time per encoder, no device-wide wait,
 * nothing on the null stream -- as hh_encoder_encode_blocks.
 * HH_ERR_ARG: a null pointer, d_offs or d_items off an 8-byte or d_out off a
 * 4-byte boundary; a symbol absent from the tree; an offs that breaks one of
 * its three rules (found on the device, in the pass over the records) -- the
 * output is untouched then and *total_bytes = 0.  HH_ERR_CAPACITY:
 * *total_bytes > cap, found before any byte of the output is written; items,
 * d_items and *total_bytes are filled (the size to retry with).
 * HH_ERR_UNSUPPORTED: nrec >= 2^32 - 1, more chunks of 4096 symbols than a
 * launch's grid holds (n above about 2^36), codes over 64 bits.  n == 0:
 * offs must be all zero; HH_OK, *total_bytes = 0, nothing written.
 * The consumer at this grain is hh_decode_batch_take: chosen records,
 * packed.  Range reads by byte offset (hh_decode_blocks_read, _gather) still
 * need one block_syms and do not take a ragged list. */
uint64_t hh_encode_ragged_bound(const hh_tree *tree, uint64_t n, uint64_t nrec);
int hh_encode_ragged(const hh_tree *tree, const uint8_t *syms, uint64_t n,
                     const uint64_t *offs /* host, nrec + 1 */, uint64_t nrec, uint8_t *out, uint64_t cap,
                     hh_batch_item *items /* host, nrec, may be NULL */, uint64_t *total_bytes);
int hh_encoder_encode_ragged(hh_encoder *enc, const hh_tree *tree, const void *d_syms, uint64_t n,
                             const uint64_t *d_offs /* device, nrec + 1 */, uint64_t nrec,
                             void *d_out, uint64_t cap,
                             hh_batch_item *d_items /* device, nrec, may be NULL */,
                             hh_batch_item *items /* host, nrec, may be NULL */,
                             uint64_t *total_bytes, void *hip_stream);
/* Compress into records: the histogram of all n > 0 bytes, hh_tree_build,
 * then hh_encoder_encode_ragged with that one tree, which *tree receives
 * (also with HH_ERR_CAPACITY).  The total bits must equal the histogram's sum
 * of count x code length, else HH_ERR_INTERNAL.  n == 0 or nrec == 0:
 * HH_ERR_ARG.  hh_compress_ragged_bound(n, nrec) = (n + 3) / 4 * 4 + 4 * nrec
 * always suffices, by hh_compress_blocks_bound's argument: the text under
 * its own Huffman code is at most 8 n bits, and rounding a record up to a
 * whole word adds less than 4 bytes. */
uint64_t hh_compress_ragged_bound(uint64_t n, uint64_t nrec);
int hh_compress_ragged_device(hh_encoder *enc, const void *d_syms, uint64_t n,
                              const uint64_t *d_offs /* device, nrec + 1 */, uint64_t nrec,
                              void *d_out, uint64_t cap, hh_tree_buf *tree,
                              hh_batch_item *d_items /* device, nrec, may be NULL */,
                              hh_batch_item *items /* host, nrec, may be NULL */,
                              uint64_t *total_bytes, void *hip_stream);

/* ---------------------------------------------------------------------- */
/* Segments (multi-GPU shards).  The stream is cut into tiles of           */
/* hh_decoder_tile_bits() bits; a segment is a run of whole tiles.  The    */
/* chain enters a segment in a STATE that is the state leaving the       */
/* previous segment; the stream starts in state 0.  States are opaque     */
/* 32-bit values of the decoder's (a node of the code tree on the state-  */
/* machine path): pass a predecessor's leave_state on unchanged, for the  */
/* same tree.  A segment's output is the symbols from its entry point up to */
/* its successor's, i.e. the segments' outputs concatenate to the stream's */
/* (the reference has no multi-device path).              */
/* ---------------------------------------------------------------------- */
int hh_decoder_tile_bits(const hh_decoder *dec, uint64_t *tile_bits);

typedef struct {
    uint64_t bits_avail;     /* readable stream bits at d_data: the segment's
                                tiles plus at least one tile after them (the
                                next segment's first regions), or up to the
                                end of the stream for the last segment     */
    uint64_t ntiles;         /* tiles to decode (prologue included; at most */
                             /* the tiles of bits_avail).  0 decodes none:  */
                             /* out_len 0, leave_state = entry_state =      */
                             /* in_state, entry_exact = (prologue == 0)     */
    uint64_t prologue;       /* the first `prologue` tiles are the end of   */
                             /* the PREVIOUS segment: decoded only to find  */
                             /* the state entering tile `prologue`, where   */
                             /* output starts (0: start at tile 0)          */
    uint32_t in_state;       /* state entering tile 0                       */
} hh_range;

typedef struct {
    uint64_t out_len;        /* symbols written                             */
    uint32_t leave_state;    /* state leaving the last tile                 */
    uint32_t const_seen;     /* 1: leave_state does not depend on the entry */
                             /* (some emitted tile's table is CONST; on the */
                             /* state machine: the entry's chain was seen   */
                             /* to meet a head's, i.e. a segment of more    */
                             /* than one count tile)                        */
    uint32_t entry_state;    /* state entering the first emitted tile       */
    uint32_t entry_exact;    /* 1: the entry state of the first emitted     */
                             /* tile is exact (no prologue, or some         */
                             /* prologue tile's table is CONST)             */
} hh_range_out;

/* Decode a segment (device pointers, stream as hh_decode_device).  A
 * shard that holds the last tiles of its predecessor before its own decodes
 * them as a prologue (in_state 0) and so finds its own entry state locally
 * (exact whenever one of those tiles is CONST, which real codes almost
 * always are); hh_range_out lets the caller check the entries against the
 * predecessors' leave_state and redo a segment entered wrongly.  Trees
 * the fused path does not handle (codes longer than 32 bits, codes that
 * never resynchronise) return HH_ERR_UNSUPPORTED: decode those whole. */
int hh_decode_device_range(hh_decoder *dec, const void *d_data, const hh_range *rg,
                           void *d_out, uint64_t cap, hh_range_out *out,
                           void *hip_stream);
/* Asynchronous form (as hh_decode_device_async): enqueues the segment's
 * decode and returns; *out is complete once the decode has been checked --
 * by the next asynchronous decode on this decoder or by hh_decode_wait,
 * which returns the first failure (HH_ERR_UNSUPPORTED for a code that does
 * not resynchronise).  const_seen and entry_exact are set at once.  *out
 * and the buffers must stay valid until hh_decode_wait returns. */
int hh_decode_device_range_async(hh_decoder *dec, const void *d_data, const hh_range *rg,
                                 void *d_out, uint64_t cap, hh_range_out *out,
                                 void *hip_stream);

/* Host-to-host convenience: H2D, hh_decode_device, D2H.  This is the scope
 * the reference times in evaluate() (decodeUtil.c:41-43). */
int hh_decode_host(hh_decoder *dec, const uint8_t *data, uint64_t bits,
                   uint8_t *out, uint64_t cap, uint64_t *out_len);
/* Releases the host buffers HH_FLAG_KEEP_HOST_PINNED kept page-locked
 * (nothing to do without the flag). */
int hh_decoder_release_host(hh_decoder *dec);

/* ---------------------------------------------------------------------- */
/* Measurement helper (not on the decode path): a streaming device-to-    */
/* device copy of nbytes (a multiple of 16, 16-B aligned pointers), 16 B  */
/* per lane, plain (nt = 0) or nontemporal (nt = 1) loads and stores; *ms */
/* gets its device time.  bench.py's reference for the HBM rate a plain  */
/* stream reaches on the same GPU (roofline.frac_vs_copy).  Returns when  */
/* done.                                                                  */
/* ---------------------------------------------------------------------- */
int hh_copy_device(const void *d_src, void *d_dst, uint64_t nbytes, int nt,
                   void *hip_stream, float *ms);

/* ---------------------------------------------------------------------- */
/* Reference-shaped stage kernels (one HIP kernel per reference kernel,   */
/* int32 arrays exactly as pes.c / the .cl kernels lay them out).  For    */
/* parity of intermediate arrays; O(25 * bits) memory, bits < 2^31.       */
/* All pointers are device pointers.                                      */
/* ---------------------------------------------------------------------- */
/* initbitsindex.cl:4-12 */
int hh_stage_initbitsindex(hh_decoder *dec, int32_t *d_bitsindex, int64_t bits,
                           void *hip_stream);
/* decodeallbits.cl:10-33: sym per bit, level-0 lengths into d_steps[0..bits) */
int hh_stage_decodeallbits(hh_decoder *dec, const void *d_data, int64_t bits,
                           uint8_t *d_bitdecode, int32_t *d_steps, void *hip_stream);
/* makebigtable.cl:10-40: level `step` -> step+1; *flag gets steps[step][0] */
int hh_stage_makebigtable(hh_decoder *dec, int64_t bits, int32_t *d_steps,
                          int32_t step, int32_t *flag, void *hip_stream);
/* calcbitsindex.cl:5-22 */
int hh_stage_calcbitsindex(hh_decoder *dec, int64_t bits, int32_t *d_bitsindex,
                           const int32_t *d_steps, int32_t step, int32_t powertwo,
                           void *hip_stream);
/* calcresult.cl:5-19 */
int hh_stage_calcresult(hh_decoder *dec, int64_t bits, const int32_t *d_bitsindex,
                        const uint8_t *d_bitdecode, uint8_t *d_result,
                        void *hip_stream);
/* findmax.cl:2-8 (parallel max-reduction instead of one work-item) */
int hh_stage_findmax(hh_decoder *dec, int64_t bits, const int32_t *d_bitsindex,
                     int32_t *maxvalue, void *hip_stream);
/* The six stages driven like openclApproach; returns the output length. */
int hh_stage_pipeline(hh_decoder *dec, const void *d_data, int64_t bits,
                      uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                      void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
