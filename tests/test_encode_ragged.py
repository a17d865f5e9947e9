"""The ragged blocked encode on the host: records cut at an offsets list
(hh_encode_ragged, hh_encode_ragged_bound, hh_compress_ragged_bound;
Tree.encode_ragged), the reference the device call (csrc/hh_encr.hip,
tests/test_gpu_encode_ragged.py) is compared with -- against one Tree.encode
per record, against Tree.encode_blocks on uniform cuts, and decoded back by
the oracle; the bounds; the statuses.  Then the emulator
(tests/emu/hh_encr_emu.cpp), which runs the device call's launches chunk by
chunk with csrc/hh_encr_algo.h's rules, against that reference on the shapes
the kernels can go wrong at.  No GPU."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import huffmandecoderongpus_amd as H
import edge_cases as E
from test_encode_blocks import strain_text
from test_gpu_encode import _random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libhh_emu.so")
NTEXT = 3 * 12289 + 1


def code_lengths(c):
    """len[256] of the code (0: absent)."""
    L = np.zeros(256, np.int64)
    for s, d in E._lengths(c.izero, c.ione, c.sym).items():
        L[s] = d
    return L


def model_items(lens, text, offs):
    """The items by the contract, vectorised: bits from the prefix sums of
    the code lengths, data_off from those of ceil(bits / 32)."""
    offs = np.asarray(offs, np.int64)
    cum = np.concatenate([[0], np.cumsum(lens[text])])
    bits = cum[offs[1:]] - cum[offs[:-1]]
    words = (bits + 31) // 32
    doff = 4 * (np.cumsum(words) - words)
    items = np.stack([doff, bits, offs[:-1], offs[1:] - offs[:-1]], axis=1).astype(np.uint64).reshape(-1, 4)
    return items, int(4 * words.sum())


def pack_records(tree, text, offs):
    """(data + pad, items): every record encoded on its own by Tree.encode, at
    4-byte boundaries; an empty record takes nothing."""
    enc = [tree.encode(text[a:b]) for a, b in zip(offs[:-1], offs[1:])]
    at, rows = 0, []
    for (p, b), a, e in zip(enc, offs[:-1], offs[1:]):
        rows.append([at, b, a, e - a])
        at += (b + 31) // 32 * 4
    data = np.zeros(at + H.PAYLOAD_PAD, np.uint8)
    for (p, b), row in zip(enc, rows):
        data[row[0]: row[0] + (b + 7) // 8] = p[: (b + 7) // 8]
    return data, np.array(rows, np.uint64).reshape(-1, 4)


def raw_ragged(tree, text, offs, cap, fill=0xAB):
    """hh_encode_ragged into a buffer of cap + 64 bytes of `fill` -> (rc, buffer, items, total)."""
    text = np.ascontiguousarray(text, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    out = np.full(cap + 64, fill, np.uint8)
    items = np.full((offs.size - 1, 4), 77, np.uint64)
    total = C.c_uint64(77)
    rc = H.lib().hh_encode_ragged(C.byref(tree._c), text.ctypes.data, text.size, offs.ctypes.data, offs.size - 1,
                                  out.ctypes.data, cap, items.ctypes.data, C.byref(total))
    return rc, out, items, int(total.value)


def random_cuts(rng, n, nrec, empties=0.2):
    """nrec records over n symbols: sorted random offsets, a share of them
    repeated (empty records)."""
    inner = np.sort(rng.integers(0, n + 1, size=nrec - 1)) if nrec > 1 else np.zeros(0, np.int64)
    if inner.size > 2:
        k = rng.random(inner.size - 1) < empties
        inner[1:][k] = inner[:-1][k]
        inner = np.sort(inner)
    return np.concatenate([[0], inner, [n]]).astype(np.uint64)


def from_lengths(lengths, n):
    """Offsets of records of these lengths, the rest of the n symbols one more."""
    o = np.concatenate([[0], np.cumsum(lengths)])
    assert o[-1] <= n
    return (np.concatenate([o, [n]]) if o[-1] < n else o).astype(np.uint64)


def shapes(n=NTEXT):
    """name -> offsets over n symbols (n no multiple of 4096): where the
    chunk geometry and the tiled scan take another path."""
    assert n % 4096 and n >= 3 * 12289
    rng = np.random.default_rng(4096)
    S = {"edges": from_lengths([15, 16, 17, 4095, 4096, 4097, 12289], n),
         "three_chunks": from_lengths([100, 3 * 4096 + 50], n),
         "empties_start": from_lengths([0, 0, 0, 5, 0, 4091], n),
         "empties_end": np.concatenate([from_lengths([7000], n), [n, n, n]]).astype(np.uint64),
         "empties_chunk_edge": from_lengths([4096, 0, 0, 0, 4095, 0, 1, 0, 0, 4097, 0], n),
         "empties_1500": from_lengths([5000] + [0] * 1500 + [3192, 1] + [0] * 1500, n),
         "ones_4096": from_lengths([1] * 8192, n)}
    for nrec in (1, 1023, 1024, 1025):
        S[f"nrec_{nrec}"] = random_cuts(rng, n, nrec)
    return S


def uniform(n, B):
    """offs[r] = min(n, r * B): hh_encode_blocks' cut."""
    return np.minimum(np.arange(-(-n // B) + 1, dtype=np.int64) * B, n).astype(np.uint64)


@pytest.fixture(scope="module")
def r40():
    """The 40-leaf random tree and an i.i.d. text of 3 * 12289 + 1 symbols."""
    rng = np.random.default_rng(12289)
    iz, io, sy, syms = _random_tree(rng, 40)
    p = rng.dirichlet(np.full(40, 0.5))
    c = SimpleNamespace(izero=iz, ione=io, sym=sy, tree=H.Tree(iz, io, sy), leaves=set(int(v) for v in syms))
    c.lens = code_lengths(c)
    return c, rng.choice(syms, size=NTEXT, p=p).astype(np.uint8)


@pytest.fixture(scope="module")
def cat64():
    iz, io, sy, text = E.every_offset_text(64)
    c = SimpleNamespace(izero=iz, ione=io, sym=sy, tree=H.Tree(iz, io, sy))
    c.lens = code_lengths(c)
    return c, text


# ---------------------------------------------------------------------------
# The host reference
# ---------------------------------------------------------------------------
def test_host_against_model(r40):
    """Random cuts (empties among them): bytes, zero padding and items are
    those of one Tree.encode per record; every record's payload decodes to its
    symbols through the oracle; the vectorised items model agrees."""
    c, full = r40
    rng = np.random.default_rng(7)
    for n, nrec in ((0, 1), (0, 3), (1, 1), (1, 4), (700, 1), (700, 40), (4100, 90), (9000, 25)):
        text = full[:n]
        offs = random_cuts(rng, n, nrec)
        data, items = c.tree.encode_ragged(text, offs)
        want, witems = pack_records(c.tree, text, offs.astype(np.int64))
        assert items.dtype == np.uint64 and np.array_equal(items, witems), (n, nrec)
        assert data.size == want.size and np.array_equal(data, want), (n, nrec)
        mitems, mtotal = model_items(c.lens, text, offs)
        assert np.array_equal(items, mitems) and data.size - H.PAYLOAD_PAD == mtotal
        assert H.encode_ragged_bound(c.tree, n, nrec) >= mtotal
        for o, b, oo, k in items.tolist():
            if k:
                assert np.array_equal(E.oracle_prefix(c, data[o:], b), text[oo: oo + k]), (n, nrec, oo)
            else:
                assert b == 0


@pytest.mark.parametrize("B", [1, 17, 4096, 4097])
def test_uniform_cuts_are_the_blocks(r40, B):
    c, full = r40
    for n in (1, B, B + 1, 3 * B + 1, 9000):
        text = full[:n]
        data, items = c.tree.encode_ragged(text, uniform(n, B))
        want, witems = c.tree.encode_blocks(text, B)
        assert np.array_equal(items, witems) and np.array_equal(data, want), (n, B)


def test_encode_bound_longest_code(cat64):
    """All-one-symbol records of the longest code (64 bits): the bound holds
    on one-symbol records, on random cuts and with empties."""
    c, _ = cat64
    n = 3000
    text = np.full(n, 63, np.uint8)
    rng = np.random.default_rng(3)
    for offs in (uniform(n, 1), uniform(n, 7), random_cuts(rng, n, 200), random_cuts(rng, n, 5000, 0.5)):
        _, items = c.tree.encode_ragged(text, offs, cap=8 * n + 4 * offs.size)
        total = int(items[-1, 0]) + (int(items[-1, 1]) + 31) // 32 * 4
        bound = H.encode_ragged_bound(c.tree, n, offs.size - 1)
        assert bound == ((n * 64 + 7) // 8 + 4 * (offs.size - 1) + 3) // 4 * 4
        assert total <= bound
    bad = H.Tree(np.array([-1], np.int32), np.array([-1], np.int32), np.array([0], np.uint8))
    assert H.lib().hh_encode_ragged_bound(bad._c, 10, 5) == 0


def test_compress_bound_rare_record():
    """One shared code: the record of the rare symbols costs more than 8 bits
    per symbol and the ragged stream still fits hh_compress_ragged_bound."""
    text = strain_text(64)
    n = text.size
    tree = H.Tree.from_counts(np.bincount(text, minlength=256))
    rng = np.random.default_rng(5)
    for head in (uniform(n - 64, 64), random_cuts(rng, n - 64, 300), random_cuts(rng, n - 64, 2000, 0.5)):
        offs = np.concatenate([head, [n]]).astype(np.uint64)
        data, items = tree.encode_ragged(text, offs)
        assert int(items[-1, 3]) == 64 and int(items[-1, 1]) > 8 * 64
        bound = H.compress_ragged_bound(n, offs.size - 1)
        assert bound == (n + 3) // 4 * 4 + 4 * (offs.size - 1)
        assert data.size - H.PAYLOAD_PAD <= bound


def test_arg_rules_leave_the_output(r40):
    """offs[0] != 0, offs[nrec] != n, a decreasing pair, an absent symbol: -1
    each, total 0 and not a byte of the output written."""
    c, full = r40
    text = full[:1000].copy()
    good = from_lengths([10, 0, 300, 90], 1000)
    rc, out, _, total = raw_ragged(c.tree, text, good, 4000)
    assert rc == 0 and 0 < total <= 4000 and (out[total:] == 0xAB).all()
    for what, offs in (("first", [1, 10, 1000]), ("last", [0, 10, 999]), ("last_over", [0, 10, 1001]),
                       ("decreasing", [0, 500, 499, 1000])):
        rc, out, _, total = raw_ragged(c.tree, text, np.array(offs, np.uint64), 4000)
        assert rc == -1 and total == 0 and (out == 0xAB).all(), what
    text[777] = next(v for v in range(256) if v not in c.leaves)
    rc, out, _, total = raw_ragged(c.tree, text, good, 4000)
    assert rc == -1 and total == 0 and (out == 0xAB).all()
    with pytest.raises(H.HipHuffError) as e:
        c.tree.encode_ragged(text, good)
    assert e.value.status == -1


def test_capacity(r40):
    c, full = r40
    text = full[:5000]
    offs = random_cuts(np.random.default_rng(11), 5000, 60)
    data, items = c.tree.encode_ragged(text, offs)
    total = data.size - H.PAYLOAD_PAD
    rc, out, it, tot = raw_ragged(c.tree, text, offs, total)          # exactly enough
    assert rc == 0 and tot == total and np.array_equal(out[:total], data[:total]) and (out[total:] == 0xAB).all()
    assert np.array_equal(it, items)
    rc, out, it, tot = raw_ragged(c.tree, text, offs, total - 1)      # one byte short: the size to retry with
    assert rc == -5 and tot == total and np.array_equal(it, items) and (out == 0xAB).all()
    with pytest.raises(H.HipHuffError) as e:
        c.tree.encode_ragged(text, offs, cap=total - 1)
    assert e.value.status == -5 and e.value.total_bytes == total and np.array_equal(e.value.items, items)


# ---------------------------------------------------------------------------
# The emulator: the device call's plan on the CPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remu():
    if not os.path.exists(EMU):
        pytest.skip("tests/emu/libhh_emu.so not built (make emu)")
    L = C.CDLL(EMU)
    if not hasattr(L, "hh_encr_emu"):
        pytest.fail("tests/emu/libhh_emu.so has no ragged encode (make emu)")
    L.hh_encr_emu.restype = C.c_int32
    L.hh_encr_emu.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.hh_encr_record_of.restype = C.c_uint64
    L.hh_encr_record_of.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.hh_encr_lower.restype = C.c_uint64
    L.hh_encr_lower.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.hh_encr_img_alloc.restype = C.c_uint32
    L.hh_encr_img_alloc.argtypes = [C.c_uint32, C.c_uint64]
    return L


def run_emu(L, c, text, offs, cap, reverse=0):
    text = np.ascontiguousarray(text, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    out = np.full(cap + 64, 0xAB, np.uint8)
    items = np.full((offs.size - 1, 4), 77, np.uint64)
    total = C.c_uint64(77)
    info = np.zeros(3, np.uint64)
    iz, io, sy = (np.ascontiguousarray(c.izero, np.int32), np.ascontiguousarray(c.ione, np.int32),
                  np.ascontiguousarray(c.sym, np.uint8))
    rc = L.hh_encr_emu(iz.ctypes.data, io.ctypes.data, sy.ctypes.data, iz.size, text.ctypes.data, text.size,
                       offs.ctypes.data, offs.size - 1, out.ctypes.data, cap, items.ctypes.data, C.byref(total),
                       reverse, info.ctypes.data)
    return rc, out, items, int(total.value), info


def emu_equals_host(L, c, text, offs):
    """The emulator into 0xAB with exactly the host's total as capacity,
    chunks first to last and last to first: bytes, items and total the
    host's (and the vectorised model's), nothing written beyond."""
    mitems, mtotal = model_items(c.lens, text, offs)
    rc, want, witems, wtotal = raw_ragged(c.tree, text, offs, mtotal)
    assert rc == 0 and wtotal == mtotal and np.array_equal(witems, mitems)
    info = None
    for reverse in (0, 1):
        rc, out, items, total, info = run_emu(L, c, text, offs, mtotal, reverse)
        assert rc == 0 and total == mtotal and not info[2], (rc, total, mtotal, info)
        assert np.array_equal(items, witems)
        assert np.array_equal(out[:total], want[:total]), int(np.argmax(out[:total] != want[:total]))
        assert (out[total:] == 0xAB).all()
    return info


def test_rules(remu):
    """The record of a symbol (the upper bound minus 1: the last of a run of
    empties) and the first record at or after a symbol, against numpy."""
    rng = np.random.default_rng(1)
    for n, nrec in ((1, 1), (50, 7), (50, 200), (5000, 300)):
        offs = random_cuts(rng, n, nrec, 0.5)
        for i in list(range(min(n, 60))) + [n - 1]:
            assert remu.hh_encr_record_of(offs.ctypes.data, nrec, i) == np.searchsorted(offs, i, side="right") - 1
        for t in list(range(min(n, 60))) + [n]:
            assert remu.hh_encr_lower(offs.ctypes.data, nrec, t) == np.searchsorted(offs[:nrec], t, side="left")
    assert remu.hh_encr_img_alloc(64, 1 << 20) == (31 + 4096 * 64 + 31 * 4096 + 31) // 32 + 1
    assert remu.hh_encr_img_alloc(19, 10) == (31 + 4096 * 19 + 31 * 10 + 31) // 32 + 1


@pytest.mark.parametrize("name", sorted(shapes()))
def test_emu_shapes(remu, r40, name):
    c, text = r40
    emu_equals_host(remu, c, text, shapes()[name])


def test_emu_worst_image(remu, cat64):
    """4096 one-symbol records in one chunk with codes of 1..64 bits: up to
    31 bits of padding after every symbol, inside the image's bound."""
    c, full = cat64
    n = 2 * 4096 + 5
    text = full[:n]
    info = emu_equals_host(remu, c, text, uniform(n, 1))
    assert 0 < info[0] <= remu.hh_encr_img_alloc(64, n)
    text = np.full(n, 32, np.uint8)                     # 33-bit codes: 31 bits of padding each
    info = emu_equals_host(remu, c, text, uniform(n, 1))
    assert info[0] == 2 * 4096
    info = emu_equals_host(remu, c, np.full(n, 63, np.uint8), from_lengths([3, 4096 * 2 - 1], n))
    assert info[0] >= 4096 * 2                          # (64-bit codes, one record over the chunk)


def test_emu_million_records(remu, r40):
    """nrec = 1024 * 1024 + 1025 one-symbol and empty records: the record
    scan's top takes its second step."""
    c, text = r40
    nrec = 1024 * 1024 + 1025
    text = np.tile(text, 9)[:300001]
    rng = np.random.default_rng(9)
    full = np.zeros(nrec, np.int64)
    full[rng.choice(nrec, size=text.size, replace=False)] = 1
    offs = np.concatenate([[0], np.cumsum(full)]).astype(np.uint64)
    info = emu_equals_host(remu, c, text, offs)
    assert info[1] == 2


def test_emu_statuses(remu, r40):
    """The device call's statuses on the emulator: each offs rule (a
    decreasing pair in the second scan tile too) and an absent symbol give -1
    with the output untouched; capacity short by a word gives -5 with items
    and total; n == 0."""
    c, full = r40
    text = full[:9000].copy()
    good = random_cuts(np.random.default_rng(2), 9000, 1500, 0.1)
    witems, total = model_items(c.lens, text, good)
    for what in ("first", "last", "pair", "pair_tile2"):
        offs = good.copy()
        if what == "first":
            offs[0] = 1
        elif what == "last":
            offs[-1] = 8999
        elif what == "pair":
            offs[10], offs[11] = 400, 399
        else:
            offs[1100], offs[1101] = offs[1101] + 1, offs[1100]
        rc, out, _, tot, info = run_emu(remu, c, text, offs, total)
        assert rc == -1 and tot == 0 and int(info[2]) & 2 and (out == 0xAB).all(), what
    rc, out, items, tot, _ = run_emu(remu, c, text, good, total - 4)
    assert rc == -5 and tot == total and np.array_equal(items, witems) and (out == 0xAB).all()
    text[4500] = next(v for v in range(256) if v not in c.leaves)
    rc, out, _, tot, info = run_emu(remu, c, text, good, total)
    assert rc == -1 and tot == 0 and int(info[2]) & 1 and (out == 0xAB).all()
    for nrec in (0, 3):
        rc, out, items, tot, _ = run_emu(remu, c, text[:0], np.zeros(nrec + 1, np.uint64), 64)
        assert rc == 0 and tot == 0 and (out == 0xAB).all() and not items[:nrec].any()
    rc, _, _, tot, _ = run_emu(remu, c, text[:0], np.array([0, 1], np.uint64), 64)
    assert rc == -1 and tot == 0
