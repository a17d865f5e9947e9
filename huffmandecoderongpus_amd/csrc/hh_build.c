/*
 * hh_build.c -- Huffman tree from byte counts (host C): the step between the
 * histogram (csrc/hh_hist.hip) and the encoder (csrc/hh_encode.hip).
 *
 * Deterministic, and node for node the tree synth.huffman_tree returns (the
 * Python heapq helper of the benchmark's byte-alphabet workload), so streams
 * made with either builder are identical:
 *   items   the symbols with counts[s] > 0 (k of them), then the internal
 *           nodes in the order they are created;
 *   key     (count, order, kind): a leaf's order is its symbol value, the
 *           i-th internal node's is k + i; kind 0 = leaf, 1 = internal (a
 *           leaf's symbol value can equal an internal node's order: the leaf
 *           goes first, as the heap's tuple comparison has it);
 *   merge   the two smallest keys a, b leave; a node of count a + b with
 *           zero-child a and one-child b enters;
 *   layout  pre-order from the root (node 0), zero subtree first; leaves
 *           izero = ione = -1, internal nodes sym = 0.
 * One distinct symbol s: root, leaf s on the zero side, leaf (s + 1) & 255 on
 * the one side (hh_tree_check rejects a root leaf).  At most 256 leaves, so
 * a plain scan for the two smallest keys (255 merges x 511 items) does.
 * No limit on the code length here: the encoder answers HH_ERR_UNSUPPORTED
 * for codes longer than 64 bits (build_codebook, hh_huff.c).
 */
#include "hiphuff.h"

#include <string.h>

typedef struct {
    uint64_t count;
    int32_t order;
    int32_t zero, one;      /* child items, -1: a leaf */
    uint8_t sym;
    uint8_t live;
} build_item;

static int key_less(const build_item *a, const build_item *b) {
    if (a->count != b->count) return a->count < b->count;
    if (a->order != b->order) return a->order < b->order;
    return a->zero < 0 && b->zero >= 0;
}

/* the live item with the smallest key (removed), -1 if none */
static int take_min(build_item *it, int n) {
    int best = -1;
    for (int i = 0; i < n; i++)
        if (it[i].live && (best < 0 || key_less(&it[i], &it[best]))) best = i;
    if (best >= 0) it[best].live = 0;
    return best;
}

int hh_tree_build(const uint64_t counts[256], hh_tree_buf *out) {
    if (!counts || !out) return HH_ERR_ARG;
    memset(out, 0, sizeof(*out));
    build_item it[HH_BUILD_MAX_NODES];
    int n = 0;
    uint64_t total = 0;
    for (int s = 0; s < 256; s++) {
        if (!counts[s]) continue;
        if (total + counts[s] < total) return HH_ERR_ARG;   /* (the total overflows) */
        total += counts[s];
        build_item leaf = {counts[s], s, -1, -1, (uint8_t)s, 1};
        it[n++] = leaf;
    }
    if (n == 0) return HH_ERR_ARG;
    const int k = n;
    int root;
    if (k == 1) {
        build_item twin = {0, 0, -1, -1, (uint8_t)((it[0].sym + 1) & 255), 0};
        build_item top = {it[0].count, 0, 0, 1, 0, 0};
        it[1] = twin;
        it[2] = top;
        n = 3;
        root = 2;
    } else {
        for (int i = 0; i + 1 < k; i++) {
            const int a = take_min(it, n), b = take_min(it, n);
            build_item node = {it[a].count + it[b].count, k + i, a, b, 0, 1};
            it[n++] = node;
        }
        root = n - 1;
    }
    /* pre-order: the one-child pushed first, so that the zero subtree's
     * nodes come before it */
    int32_t stk[HH_BUILD_MAX_NODES], par[HH_BUILD_MAX_NODES];
    int sp = 0;
    int32_t nodes = 0;
    stk[sp] = root; par[sp] = -1; sp++;
    while (sp) {
        sp--;
        const build_item *x = &it[stk[sp]];
        const int32_t v = nodes++, p = par[sp];
        if (p >= 0) {
            /* (a parent's zero-child is the node right after it) */
            if (v == p + 1) out->izero[p] = v;
            else out->ione[p] = v;
        }
        out->izero[v] = out->ione[v] = -1;
        out->sym[v] = x->sym;
        if (x->zero >= 0) {
            stk[sp] = x->one; par[sp] = v; sp++;
            stk[sp] = x->zero; par[sp] = v; sp++;
        }
    }
    out->nodes = nodes;
    return HH_OK;
}
