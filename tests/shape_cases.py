"""The shape family: trees chosen for the geometry hh_decoder_set_tree derives
from them, beside edge_cases' CODE_NAMES, which are chosen for the launch
shapes of long streams (and parametrize the 2049-tile tests: the shapes take
no part in those).  A plain helper module as edge_cases is (no fixtures, no
GPU): tests/test_emu_shapes.py runs the shapes through the emulators,
tests/test_gpu_batch_shapes.py on the GPU.

Beside the family it holds the few helpers of the batch tests that take a
code's name, in a form that takes a shape's as well (stream, blocked, and the
bodies of the two emulator tests with the emission step as a parameter); for
the names of CODE_NAMES they give what the originals give."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import edge_cases as E
from edge_cases import CODE_NAMES, FLAG_NO_FIXED, NR, Code, _lengths, _tail_bytes
from test_gpu_parity import _caterpillar, _complete_tree, _random_tree

# ---------------------------------------------------------------------------
# The shape family: trees chosen for the geometry hh_decoder_set_tree derives
# from them (region bits S, emission step K, remainder step r = S mod K,
# count step bits cb, the batch's head G, its waves per round W), not for
# their launch shapes.  SHAPE_GEOMETRY is what Decoder.geometry() reports for
# each (tests/test_gpu_batch_shapes.py::test_geometry_cells holds the library
# to it; DESIGN.md section 9 sets it beside the host replay it was predicted
# from).
# ---------------------------------------------------------------------------
SHAPE_NAMES = ("complete5", "complete7", "complete8", "lattice3", "lattice5", "lattice6", "split7", "random128",
               "random200", "random12", "caterpillar64")

#                 name            S    K  r  cb   G   W   ns
SHAPE_GEOMETRY = {"complete5":     (160, 7, 6, 8,   0, 16,  31),
                  "complete7":     (224, 6, 2, 8,   0, 16, 127),
                  "complete8":     (224, 5, 4, 7,   0, 16, 255),
                  "lattice3":      (192, 7, 3, 8, 126, 16,  14),
                  "lattice5":      (160, 7, 6, 8, 105, 16,  62),
                  "lattice6":      (192, 6, 0, 8, 126, 16, 126),
                  "split7":        (224, 6, 2, 7, 126, 16, 128),
                  "random128":     (256, 6, 4, 8, 126, 12, 127),
                  "random200":     (224, 6, 2, 7, 126,  8, 199),
                  "random12":      (256, 7, 4, 8, 126, 14,  11),
                  "caterpillar64": (256, 4, 0, 8, 128,  7,  64)}
CODE_GEOMETRY = {"kjv":           (256, 7, 4, 8, 126,  6,  83),
                 "byte256":       (224, 5, 4, 7, 125,  6, 255),
                 "fixed2":        (128, 7, 2, 8,   0, 16,   3),
                 "fixed1":        (64, 4, 0, 8,   0, 16,   1),
                 "caterpillar40": (256, 4, 0, 8, 128,  8,  40)}
GEOMETRY_KEYS = ("S", "K", "r", "cb", "G", "W", "ns")


def _grafted(depth, sub):
    """The complete `depth`-bit tree with its last leaf replaced by the
    complete `sub`-bit tree: code lengths depth and depth + sub, the leaves'
    symbols 0, 1, ... in node order."""
    iz, io, sy = (list(a) for a in _complete_tree(depth))
    siz, sio, _ = _complete_tree(sub)
    at = len(iz) - 1                                  # the last leaf: the subtree's root; its node j > 0 is at + j
    iz[at], io[at] = at + int(siz[0]), at + int(sio[0])
    for a, b in zip(siz[1:], sio[1:]):
        iz.append(at + int(a) if a >= 0 else -1)
        io.append(at + int(b) if b >= 0 else -1)
        sy.append(0)
    iz, io, sy = np.array(iz), np.array(io), np.array(sy)
    leaves = np.flatnonzero(iz == -1)
    assert leaves.size <= 256
    sy[leaves] = np.arange(leaves.size)
    return iz, io, sy


def _dyadic(iz, io, sy):
    """(symbols, 2^-length): the distribution the code is optimal for."""
    L = _lengths(iz, io, sy)
    s = sorted(L)
    p = np.array([2.0 ** -L[k] for k in s])
    assert abs(p.sum() - 1.0) < 1e-12
    return np.array(s, np.uint8), p / p.sum()


@functools.lru_cache(maxsize=None)
def shape(name) -> Code:
    """completeN: the complete N-bit code, through the general pipeline as
    fixed2 is; latticeN: lengths N and 2 N (gcd N: a non-fixed code on a
    lattice); split7: lengths 7 and 8, 128 states (the first tree counted in
    7-bit steps); randomN: _random_tree(default_rng(N), N); caterpillar64:
    codes of 1 .. 64 bits."""
    build = {"complete5": lambda: _complete_tree(5), "complete7": lambda: _complete_tree(7),
             "complete8": lambda: _complete_tree(8), "lattice3": lambda: _grafted(3, 3),
             "lattice5": lambda: _grafted(5, 5), "lattice6": lambda: _grafted(6, 6), "split7": lambda: _grafted(7, 1),
             "random128": lambda: _random_tree(np.random.default_rng(128), 128)[:3],
             "random200": lambda: _random_tree(np.random.default_rng(200), 200)[:3],
             "random12": lambda: _random_tree(np.random.default_rng(12), 12)[:3],
             "caterpillar64": lambda: _caterpillar(64)}
    iz, io, sy = build[name]()
    sy = _tail_bytes(iz, sy)
    fixed = name.startswith("complete")
    return Code(name, iz, io, sy, FLAG_NO_FIXED if fixed else 0, fixed, _dyadic(iz, io, sy))


def any_code(name) -> Code:
    """edge_cases.code(name) or shape(name)."""
    return E.code(name) if name in CODE_NAMES else shape(name)


def name_index(name) -> int:
    """A name's place in CODE_NAMES + SHAPE_NAMES (the seeds of its streams)."""
    return (CODE_NAMES + SHAPE_NAMES).index(name)


@functools.lru_cache(maxsize=None)
def stream(name, S, tiles):
    """edge_cases.stream for a shape as well (a name of CODE_NAMES: that very
    stream): (payload + 64 zero bytes, bits, text or None), at least tiles *
    64 S + S + 2 bits; complete codes random bytes, the others i.i.d. symbols
    of the code's distribution encoded by the host encoder."""
    if name in CODE_NAMES:
        return E.stream(name, S, tiles)
    c = shape(name)
    need = tiles * NR * S + S + 2
    rng = np.random.default_rng([S, tiles, name_index(name)])
    if c.complete:
        data = np.zeros((need + 7) // 8 + 64, np.uint8)
        data[: (need + 7) // 8] = rng.integers(0, 256, (need + 7) // 8, dtype=np.uint8)
        return data, need, None
    syms, p = c.probs
    L = _lengths(c.izero, c.ione, c.sym)
    avg = float(sum(p[i] * L[int(s)] for i, s in enumerate(syms)))
    text = rng.choice(syms, size=int(need / avg * 1.02) + 4096, p=p).astype(np.uint8)
    data, bits = c.tree().encode(text)
    assert bits >= need, (name, bits, need)
    return data, bits, text


@functools.lru_cache(maxsize=None)
def blocked(name, W, S):
    """test_gpu_blocks_read.py's _blocked for a shape: five blocks, each a
    little over three rounds of W tiles of 64 S bits, the last one short:
    (text, block_syms, payload + pad, index rows) from the host encoder."""
    c = any_code(name)
    L = _lengths(c.izero, c.ione, c.sym)
    rng = np.random.default_rng([W, S, name_index(name)])
    syms, p = c.probs
    RB = 64 * W * S
    draw = lambda n: rng.choice(syms, size=n, p=p).astype(np.uint8)
    avg = float(np.mean([L[int(s)] for s in draw(20000)]))
    B = int(3.3 * RB / avg)
    text = draw(4 * B + B // 3)
    data, index = c.tree().encode_blocks(text, B)
    assert index.shape[0] == 5 and all(3 * RB < b < 4 * RB for b in index[:4, 1].tolist()), (index, RB)
    return text, B, data, index
