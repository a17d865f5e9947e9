"""The device-side plan of the batched decode (csrc/hh_batch_plan_algo.h) on
the host: the emulator (tests/emu/hh_batch_plan_emu.cpp) compiles the very
functions k_plan_count and k_plan_place run per item -- the validity rule,
the bin key, the bins' starts -- and runs the counting sort workgroup by
workgroup.  The validity rule is what keeps a bad item from becoming an
address, so its overflow corners are checked here and never sent to a GPU.
tests/test_gpu_batch_items.py runs the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libhh_emu.so")
PAD = 64                    # HH_PAYLOAD_PAD
M64 = (1 << 64) - 1
RB = 64 * 16 * 128          # a round's bits at W = 16, S = 128


@pytest.fixture(scope="module")
def pemu():
    if not os.path.exists(EMU):
        pytest.skip("tests/emu/libhh_emu.so not built (make emu)")
    L = C.CDLL(EMU)
    L.hh_batch_plan_bins.restype = C.c_uint32
    L.hh_batch_plan_item_ok.restype = C.c_int32
    L.hh_batch_plan_item_ok.argtypes = [C.c_uint64] * 6
    L.hh_batch_plan_bin.restype = C.c_uint32
    L.hh_batch_plan_bin.argtypes = [C.c_uint64] * 2
    L.hh_batch_plan_emu.restype = C.c_int32
    L.hh_batch_plan_emu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def rule(item, data_bytes, out_bytes):
    """The header's three rules (include/hiphuff.h, hh_decode_batch_device) in
    Python's unbounded integers: nothing here can overflow."""
    d, b, o, c = item
    if d % 4:
        return False
    if b > 0 and d + (b + 7) // 8 + PAD > data_bytes:
        return False
    return o + c <= out_bytes


def bin_of(bits, nbins, rb=RB):
    return min(-(-bits // rb), nbins - 1)


def test_validity_rule(pemu):
    """The items of test_gpu_batch.py::test_arguments (4096 bytes of payload,
    1024 of output), the ends of both buffers, and the corners at which a sum
    of the rule wraps around 2^64 when computed carelessly."""
    DB, OB = 4096, 1024
    good = [[0, 256, 0, 512], [4096, 0, 1024, 0], [4028, 32, 0, 1024], [DB - 68, 32, 0, 0], [0, 0, OB, 0],
            [M64 - 3, 0, 0, 0]]                                  # (no bits: the offset is never used)
    bad = [[2, 256, 0, 512], [0, 8 * (4096 - 64) + 1, 0, 1024], [4032, 8, 0, 512], [8192, 8, 0, 512],
           [0, 256, 1000, 25], [0, 256, 1025, 0], [0, 256, 0, 1 << 63], [0, M64, 0, 512],
           [M64 - 3, 8, 0, 0],                                   # data_off + bytes wraps to a small number
           [M64 - 3, M64, 0, 0],
           [0, M64 - 6, 0, 0], [4, M64, 0, 0],                   # ceil(bits / 8) computed as (bits + 7) / 8 wraps
           [0, 8, 8, 1 << 63], [0, 8, 1 << 63, 1 << 63],          # out_off + cap wraps to 0
           [0, 8, M64, 1], [0, 8, 1, M64], [0, 8, OB, 1], [0, 8, OB + 1, 0],
           [DB - 64, 32, 0, 0], [DB - 68, 33, 0, 0], [DB, 1, 0, 0]]
    for item in good:
        assert rule(item, DB, OB), item
    for item in bad:
        assert not rule(item, DB, OB), item
    for item in good + bad:
        assert bool(pemu.hh_batch_plan_item_ok(*item, DB, OB)) == rule(item, DB, OB), item
    # the buffers themselves at the top of the address space
    for item in ([M64 - 3 - 68, 32, M64 - 8, 8], [M64 - 3 - 64, 32, 0, 0], [0, 8, M64, 0], [0, 8, M64 - 1, 2]):
        assert bool(pemu.hh_batch_plan_item_ok(*item, M64 - 3, M64)) == rule(item, M64 - 3, M64), item
    rng = np.random.default_rng(64)
    for _ in range(2000):                                        # small sizes: every rule fires often
        item = [int(rng.integers(0, 40)) * int(rng.choice([1, 4])), int(rng.integers(0, 400)),
                int(rng.integers(0, 40)), int(rng.integers(0, 40))]
        db, ob = int(rng.integers(60, 140)), int(rng.integers(0, 60))
        assert bool(pemu.hh_batch_plan_item_ok(*item, db, ob)) == rule(item, db, ob), (item, db, ob)


def test_bins(pemu):
    """The key: a stream's rounds, clamped; a bin per lane of a wave."""
    nbins = pemu.hh_batch_plan_bins()
    assert nbins == 64
    for k in list(range(0, nbins + 3)) + [1000, 1 << 40]:
        for d in (-1, 0, 1):
            bits = k * RB + d
            if 0 <= bits <= M64:
                assert pemu.hh_batch_plan_bin(bits, RB) == bin_of(bits, nbins), bits
    assert pemu.hh_batch_plan_bin(M64, RB) == nbins - 1 and pemu.hh_batch_plan_bin(M64, 1) == nbins - 1
    assert pemu.hh_batch_plan_bin(0, RB) == 0 and pemu.hh_batch_plan_bin(1, RB) == 1


def _lengths(kind, n, nbins, rng):
    if kind == "random":
        return [int(v) for v in rng.integers(0, 70 * RB, n)]
    if kind == "equal":
        return [3 * RB + 5] * n
    if kind == "edges":                                          # both sides of every bin edge and of the clamp
        v = [k * RB + d for k in range(1, nbins + 2) for d in (-1, 0, 1)] + [0, 1, 100 * RB]
        return [v[int(i)] for i in rng.permutation(len(v))][:n] if n < len(v) else \
            v + [int(x) for x in rng.integers(0, 70 * RB, n - len(v))]
    if kind == "zero":
        return [0 if k % 2 else int(rng.integers(0, 3 * RB)) for k in range(n)]
    raise ValueError(kind)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("kind", ["random", "equal", "edges", "zero"])
def test_order(pemu, kind, n):
    """The plan's list is a permutation of 0..n-1 by non-increasing bin, for
    workgroups of 64 and of 256 items reaching the bins' cursors in either
    order; an invalid item (every seventh here) keeps its index, carries the
    empty descriptor -- no offset of it survives -- and is marked in its key;
    a valid item's descriptor is the item."""
    nbins = pemu.hh_batch_plan_bins()
    rng = np.random.default_rng(n * 7 + len(kind))
    DB, OB = 80 * RB, 1 << 30
    bits = _lengths(kind, n, nbins, rng)
    items = np.array([[4 * k, b, 16 * k, 16] for k, b in enumerate(bits)], np.uint64).reshape(-1, 4)
    breaks = ([2, 8, 0, 0], [DB, 8, 0, 0], [0, 8, OB, 1], [M64 - 3, M64, M64, M64])
    for k in range(0, n, 7):
        if n > 2 or k:
            items[k] = breaks[(k // 7) % 4]
    valid = [rule([int(x) for x in it], DB, OB) for it in items]
    assert not all(valid) or n <= 2
    want_bin = [bin_of(int(it[1]), nbins) if ok else 0 for it, ok in zip(items, valid)]
    for tb in (64, 256):
        for reverse in (0, 1):
            key = np.zeros(n, np.uint8)
            order = np.full(n, 0xffffffff, np.uint32)
            desc = np.full((n, 5), 0xAB, np.uint64)
            rc = pemu.hh_batch_plan_emu(items.ctypes.data, n, DB, OB, RB, tb, reverse, key.ctypes.data,
                                        order.ctypes.data, desc.ctypes.data)
            assert rc == 0
            assert sorted(order.tolist()) == list(range(n))
            assert key.tolist() == [b if ok else 0x80 for b, ok in zip(want_bin, valid)]
            got = [want_bin[i] for i in order.tolist()]
            assert all(a >= b for a, b in zip(got, got[1:])), (tb, reverse)
            assert np.array_equal(desc[:, 4], order)
            for k, i in enumerate(order.tolist()):
                assert desc[k, :4].tolist() == (items[i].tolist() if valid[i] else [0, 0, 0, 0]), (k, i)
