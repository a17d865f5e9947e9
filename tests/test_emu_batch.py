"""The batched decode's round rules (csrc/hh_batch_algo.h) on the host: the
emulator (tests/emu/hh_batch_emu.cpp) runs k_batch's decomposition -- rounds
of W tiles, guesses, counts over the emission tables, fix rounds, scan,
emission, the copy-out clipped to each stream's capacity -- for a list of
items, against the oracle's chain decode of each stream.  tests/
test_gpu_batch.py decodes the same cuts on the GPU: a length that fails here
is wrong in the rules, one that fails only there in the kernel or its launch.
"""
import ctypes as C
import os

import numpy as np
import pytest

import edge_cases as E
from test_gpu_parity import _complete_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libhh_emu.so")
GUARD = 256
_REFS = {}                 # (code, bits) -> the oracle's decode


@pytest.fixture(scope="module")
def bemu():
    if not os.path.exists(EMU):
        pytest.skip("tests/emu/libhh_emu.so not built (make emu)")
    L = C.CDLL(EMU)
    L.hh_batch_emu_decode.restype = C.c_int64
    L.hh_batch_emu_decode.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def run_bemu(L, izero, ione, sym, data, items, out, W, S=0, K=0):
    """(rc, out_len, status, stats) of one emulated batch into out."""
    iz = np.ascontiguousarray(izero, np.int32)
    io = np.ascontiguousarray(ione, np.int32)
    sy = np.ascontiguousarray(sym, np.uint8)
    data = np.ascontiguousarray(data, np.uint8)
    items = np.ascontiguousarray(items, np.uint64).reshape(-1, 4)
    n = items.shape[0]
    out_len = np.zeros(n, np.uint64)
    status = np.zeros(n, np.int32)
    st = np.zeros(7, np.int64)
    rc = L.hh_batch_emu_decode(iz.ctypes.data, io.ctypes.data, sy.ctypes.data, len(iz), data.ctypes.data, data.size,
                               items.ctypes.data, n, S, K, W, out.ctypes.data, out.size, out_len.ctypes.data,
                               status.ctypes.data, st.ctypes.data)
    return int(rc), out_len, status, st


def batch_cuts(S, W, maxlen, limit):
    """The stream lengths of a batch for regions of S bits and rounds of W
    tiles: the first bits, bytes and words, the longest code, the first
    regions, and both sides of every tile and round boundary up to three
    rounds."""
    TB = 64 * S
    v = {1, 2, 7, 8, 9, 31, 32, 33, maxlen - 1, maxlen, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1}
    for k in (1, 2, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W):
        v.update(k * TB + d for d in (-1, 0, 1, S - 1, S, S + 1))
    return sorted(b for b in v if 1 <= b <= limit)


def _region_bits(L, c):
    out = np.zeros(64, np.uint8)
    rc, _, _, st = run_bemu(L, c.izero, c.ione, c.sym, np.zeros(128, np.uint8), [[0, 8, 0, 64]], out, 1)
    assert rc == 0
    return int(st[0])


def _ref(name, data, bits):
    r = _REFS.get((name, bits))
    if r is None:
        r = _REFS[(name, bits)] = E.oracle_prefix(E.code(name), data, bits)
    return r


@pytest.mark.parametrize("W", [1, 2, 16])
@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_batch_breakpoints(bemu, name, W):
    """One batch of every cut of batch_cuts, all prefixes of one stream
    (data_off 0: the inputs overlap), the outputs packed back to back in index
    order from out_off 1 with each capacity exactly the oracle's length: every
    stream's bytes and length are the oracle's, every status 0, and the byte
    before the first output and those after the last are untouched."""
    c = E.code(name)
    S = _region_bits(bemu, c)
    assert S % 32 == 0 and (name != "byte256" or S == 224)
    data, bits, _ = E.stream(name, S, 49)
    cuts = batch_cuts(S, W, c.tree().info()["maxlen"], bits)
    assert cuts[-1] == 3 * W * 64 * S + S + 1 and W * 64 * S in cuts
    refs = [_ref(name, data, b) for b in cuts]
    items, off = [], 1
    for b, r in zip(cuts, refs):
        items.append([0, b, off, len(r)])
        off += len(r)
    out = np.full(off + GUARD, 0xAB, np.uint8)
    rc, out_len, status, st = run_bemu(bemu, c.izero, c.ione, c.sym, data, items, out, W)
    assert rc == 0 and not status.any(), (rc, status, st)
    for (_, b, o, n), r, got in zip(items, refs, out_len):
        assert got == n and np.array_equal(out[o: o + n], r), (b, divmod(b, 64 * S), got, n)
    assert out[0] == 0xAB and (out[off:] == 0xAB).all()


def test_batch_capacity_is_per_stream(bemu):
    """Capacities of len and len - 1 in turn, 64 bytes apart: the short ones
    report HH_ERR_CAPACITY with the full length and write nothing at or beyond
    out_off + cap, the others are exact; the batch returns -5."""
    name, W = "kjv", 2
    c = E.code(name)
    S = _region_bits(bemu, c)
    data, bits, _ = E.stream(name, S, 49)
    cuts = batch_cuts(S, W, c.tree().info()["maxlen"], bits)
    refs = [_ref(name, data, b) for b in cuts]
    items, off = [], 3
    for k, (b, r) in enumerate(zip(cuts, refs)):
        items.append([0, b, off, len(r) - (k % 2)])
        off += len(r) + 64
    out = np.full(off + GUARD, 0xAB, np.uint8)
    rc, out_len, status, _ = run_bemu(bemu, c.izero, c.ione, c.sym, data, items, out, W)
    assert rc == -5
    end = 0
    for k, ((_, b, o, cap), r) in enumerate(zip(items, refs)):
        assert out_len[k] == len(r) and status[k] == (-5 if k % 2 else 0), (k, b, out_len[k], status[k])
        assert (out[end: o] == 0xAB).all(), (k, b)
        assert np.array_equal(out[o: o + cap], r[:cap]), (k, b)
        end = o + cap
    assert (out[end:] == 0xAB).all()


@pytest.mark.parametrize("W", [1, 2, 16])
def test_fix_rounds_make_a_code_that_never_resynchronises_exact(bemu, W):
    """A complete fixed-length code never resynchronises: a chain entered off
    the code's lattice stays off it.  The 7-bit complete code (127 internal
    nodes; the largest complete code off the 32-bit lattice that the state
    machine's 255 states hold -- the 11-bit one of test_gpu_parity.py::
    test_non_resynchronising_code_takes_the_segment_path has 2047 and is
    HH_ERR_UNSUPPORTED here, as in the library) with 96-bit regions: regions
    start on a code boundary every 7th time only, the guess (the root: a
    fixed-length code has no head) is wrong for the six between, and the fix
    rounds do all the work: a lane takes its predecessor's exit whenever it
    differs from its entry, a chain off the lattice never leaves a region in
    the state of one on it, so region j is right after fix round j and not
    before -- the 22 regions of a stream take exactly 21 fix rounds."""
    iz, io, sy = _complete_tree(7)
    rng = np.random.default_rng(7)
    bits = 7 * 300 + 5
    nb = (bits + 7) // 8
    blocks = [rng.integers(0, 256, nb, dtype=np.uint8) for _ in range(4)]
    stride = (nb + 3) // 4 * 4
    data = np.zeros(4 * stride + 64, np.uint8)
    items, off = [], 1
    refs = []
    from oracle import oracle as O
    for k, blk in enumerate(blocks):
        data[k * stride: k * stride + nb] = blk
        hf = O.Huff(bits, 0, iz.astype(np.int32), io.astype(np.int32), sy.astype(np.uint8), blk)
        refs.append(O.OracleHuff.from_arrays(hf).chain_decode())
        items.append([k * stride, bits, off, len(refs[-1])])
        off += len(refs[-1])
    out = np.full(off + GUARD, 0xAB, np.uint8)
    rc, out_len, status, st = run_bemu(bemu, iz, io, sy, data, items, out, W, S=96)
    assert rc == 0 and not status.any(), (rc, status, st)
    assert st[0] == 96 and st[1] == 0 and st[5] == (bits + 95) // 96 - 1 and st[6] > 0, st
    for (_, _, o, n), r, got in zip(items, refs, out_len):
        assert got == n == 301 and np.array_equal(out[o: o + n], r)
    assert out[0] == 0xAB and (out[off:] == 0xAB).all()
    iz, io, sy = _complete_tree(11)
    rc, _, _, _ = run_bemu(bemu, iz, io, sy, data, items, out, W, S=96)
    assert rc == -10


def test_batch_arguments(bemu):
    """The C ABI's argument checks, in the emulator too: a data_off off a
    4-byte boundary, a payload (with its pad) past data_bytes, an output range
    past out_bytes; an empty batch is fine."""
    c = E.code("kjv")
    data = np.zeros(256, np.uint8)
    out = np.full(128, 0xAB, np.uint8)
    for item in ([2, 64, 0, 64], [0, 8 * (256 - 64) + 1, 0, 64], [192, 8, 0, 64], [0, 64, 100, 29], [0, 64, 129, 0]):
        rc, _, _, _ = run_bemu(bemu, c.izero, c.ione, c.sym, data, [item], out, 2)
        assert rc == -1, item
    assert (out == 0xAB).all()
    rc, _, _, _ = run_bemu(bemu, c.izero, c.ione, c.sym, data, np.zeros((0, 4), np.uint64), out, 2)
    assert rc == 0
    rc, n, s, _ = run_bemu(bemu, c.izero, c.ione, c.sym, data, [[0, 0, 128, 0], [188, 32, 0, 64]], out, 2)
    assert rc == 0 and n[0] == 0 and not s.any()
