"""Stream lengths and codes at which the decoder's launch changes shape.

A plain helper module (no fixtures, no GPU): tests/test_gpu_edges.py decodes
these on the GPU, tests/test_emu_edges.py runs the same list through the kernel
emulator.

fsm_launch (csrc/hh_fsm.hip) picks its kernels and grids from the stream's
length in bits through a handful of inequalities, with S the region bits,
TB = 64 S a tile's bits and M the count pass's regions per lane (HH_CNT_M):

    bits > TB + S, (bits - S - 1) / TB   the count tiles of the main launch
    nc / M, nc < M, nt - (nc / M) M      k_cntm / k_cnt / the tail workgroups
    min(bits / TB, nt)                   main and tail emission (none when
                                         bits is a multiple of TB)
    (nt + 1 + 1023) / 1024               scan blocks; k_emf reads blk[t / 1024]
    16 tiles per workgroup               k_cnt's and k_emf's waves

breakpoint_bits lists the lengths on both sides of each of them.  It is
derived from those inequalities alone, not from what the kernels return.
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass

import numpy as np

from test_gpu_parity import _caterpillar, _complete_tree

NR = 64                                   # regions per tile
FLAG_NO_FIXED = 4
SCAN_K = (1023, 1024, 1025, 2047, 2048, 2049)   # tiles around k_fscan1's 1024-tile blocks
MAX_TILES = SCAN_K[-1]
FILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "files")


def breakpoint_bits(S, M, maxlen, limit=None, scan_k=SCAN_K, scan_d=None):
    """The sorted, de-duplicated stream lengths (bits) to decode for regions
    of S bits, M regions per lane of the count pass and codes of up to maxlen
    bits; `limit`, the stream's length, drops what lies beyond it.  scan_k
    and scan_d (offsets from k TB; default -1, 0, 1, S, S + 1) thin the rows
    around the scan blocks for the emulator."""
    TB = NR * S
    v = {1, 2, 7, 8, 9, 31, 32, 33, maxlen - 1, maxlen, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1,
         M * S, M * S + 1}
    for k in (1, 2, 3, M, M + 1, 2 * M, 2 * M + 1, 15, 16, 17, 16 * M, 16 * M + 1, 32, 33):
        v.update(k * TB + d for d in (-1, 0, 1, S - 1, S, S + 1, S + 2))
    for k in scan_k:
        v.update(k * TB + d for d in (scan_d if scan_d is not None else (-1, 0, 1, S, S + 1)))
    return sorted(b for b in v if b >= 1 and (limit is None or b <= limit))


@dataclass(frozen=True)
class Code:
    name: str
    izero: np.ndarray
    ione: np.ndarray
    sym: np.ndarray
    flags: int            # decoder flags that send it through the state machine
    complete: bool        # a complete fixed-length code: any bit string is a stream
    probs: object         # (symbols, probabilities) of the i.i.d. text, or None

    def tree(self):
        import huffmandecoderongpus_amd as H
        return H.Tree(self.izero, self.ione, self.sym)


def _tail_bytes(iz, sy):
    """Internal nodes hold distinct nonzero tail-rule bytes (a stream cut
    inside a code ends with its node's byte)."""
    sy = np.array(sy, np.uint8)
    inner = np.flatnonzero(np.asarray(iz) >= 0)
    sy[inner] = (inner * 37 + 0x81) | 0x80
    return sy


def _lengths(iz, io, sy):
    L = {}
    stack = [(0, 0)]
    while stack:
        v, d = stack.pop()
        if iz[v] == -1:
            L.setdefault(int(sy[v]), d)
        else:
            stack += [(int(iz[v]), d + 1), (int(io[v]), d + 1)]
    return L


CODE_NAMES = ("kjv", "byte256", "fixed2", "fixed1", "caterpillar40")


@functools.lru_cache(maxsize=None)
def code(name) -> Code:
    """1 kjv's tree; 2 the 256-leaf byte-alphabet Huffman tree (255 states,
    224-bit regions); 3, 4 the complete 2- and 1-bit codes through the general
    pipeline (HH_FLAG_NO_FIXED: the swizzled staging with the 16-store
    copy-out; 16384 bytes per tile, the copy-out loop); 5 the 40-deep
    caterpillar (codes longer than the table steps, crossing regions)."""
    import huffmandecoderongpus_amd as H
    from huffmandecoderongpus_amd import synth
    if name == "kjv":
        hf = H.HuffFile.load(os.path.join(FILES, "kjv.txt.huff"))
        iz, io, sy = hf.izero, hf.ione, hf.sym
        L = _lengths(iz, io, sy)
        s = sorted(L)
        p = np.array([2.0 ** -L[k] for k in s])
        return Code(name, iz, io, sy, 0, False, (np.array(s, np.uint8), p / p.sum()))
    if name == "byte256":
        counts = synth.byte_counts()
        t = synth.huffman_tree(counts)
        return Code(name, t.izero, t.ione, _tail_bytes(t.izero, t.sym), 0, False,
                    (np.arange(256, dtype=np.uint8), counts / counts.sum()))
    if name in ("fixed2", "fixed1"):
        iz, io, sy = _complete_tree(int(name[-1]))
        return Code(name, iz, io, _tail_bytes(iz, sy), FLAG_NO_FIXED, True, None)
    if name == "caterpillar40":
        iz, io, sy = _caterpillar(40)
        return Code(name, iz, io, sy, 0, False, (np.arange(41, dtype=np.uint8), np.full(41, 1 / 41)))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stream(name, S, tiles=MAX_TILES):
    """(payload + 64 zero bytes, bits, text or None): one seeded stream of
    code `name`, at least tiles * 64 S + S + 2 bits long.  Every length a test
    decodes is a prefix of it; a cut inside a code takes the reference's tail
    rule.  Complete codes: random bytes (any bit string decodes); the others:
    i.i.d. symbols encoded once by the host encoder."""
    c = code(name)
    need = tiles * NR * S + S + 2
    rng = np.random.default_rng([S, tiles, CODE_NAMES.index(name)])
    if c.complete:
        data = np.zeros((need + 7) // 8 + 64, np.uint8)
        data[: (need + 7) // 8] = rng.integers(0, 256, (need + 7) // 8, dtype=np.uint8)
        return data, need, None
    syms, p = c.probs
    L = _lengths(c.izero, c.ione, c.sym)
    avg = float(sum(p[i] * L[int(s)] for i, s in enumerate(syms)))
    n = int(need / avg * 1.02) + 4096
    text = rng.choice(syms, size=n, p=p).astype(np.uint8)
    data, bits = c.tree().encode(text)
    assert bits >= need, (name, bits, need)
    return data, bits, text


def oracle_prefix(c: Code, data, bits):
    """The oracle's chain decode of the first `bits` bits of data."""
    from oracle import oracle as O
    nb = (bits + 7) // 8
    hf = O.Huff(bits, 0, np.asarray(c.izero, np.int32), np.asarray(c.ione, np.int32),
                np.asarray(c.sym, np.uint8), np.asarray(data, np.uint8)[:nb])
    return O.OracleHuff.from_arrays(hf).chain_decode()


# ---------------------------------------------------------------------------
# The encoders' long codes: a code of l bits that starts at bit o of a 32-bit
# word spans 1, 2 or (o + l > 64) 3 words.
# ---------------------------------------------------------------------------
def every_offset_text(depth=64):
    """(izero, ione, sym, text) of the `depth`-deep caterpillar (symbol k:
    k + 1 bits, k < depth; code lengths 1..depth) and a text in which a code
    of every length l in 1..depth starts at every bit offset o in 0..31 of a
    32-bit word: the 1-bit symbol pads up to offset o, then comes the symbol
    of l bits.  The cumulative lengths are checked here: all 32 x depth
    (o, l) pairs occur."""
    iz, io, sy = _caterpillar(depth)
    text, pos = [], 0
    for l in range(1, depth + 1):
        for o in range(32):
            pad = (o - pos) % 32
            text += [0] * pad + [l - 1]
            pos += pad + l
    text = np.array(text, np.uint8)
    lens = text.astype(np.int64) + 1
    start = np.cumsum(lens) - lens
    seen = set(zip((start % 32).tolist(), lens.tolist()))
    assert all((o, l) in seen for o in range(32) for l in range(1, depth + 1))
    assert int(start[-1] + lens[-1]) == pos
    return iz, io, sy, text
