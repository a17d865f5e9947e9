"""Gathered range reads over a block-coded buffer (hh_decode_blocks_gather) on
the host: the emulator (tests/emu/hh_blocks_gather_emu.cpp) compiles the very
rules the kernels of csrc/hh_batch_gather.hip run -- the read rules of
csrc/hh_batch_read_algo.h up to the pieces, then the grouping by block, the
walk's end, a piece's result and the copy's split of
csrc/hh_batch_gather_algo.h -- and runs the plan slot by slot and k_gather's
merged walk lane by lane.  The plan is held to tests/test_blocks_read.py's
model, the walk to hh_blocks_read_emu_decode run piece by piece (which that
file holds to the oracle).  tests/test_gpu_blocks_gather.py runs the kernels."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as EC
import shape_cases as E
from test_blocks_read import ERR_ARG, ERR_FORMAT, INVALID, M64, _index, block_windows, budget, model, remu, \
    round_counts, rounds_for  # noqa: F401  (remu: a fixture)
from test_emu_shapes import GEO, run_decode

ERR_UNSUPPORTED = -10


@pytest.fixture(scope="module")
def gemu(remu):
    L = remu
    if not hasattr(L, "hh_blocks_gather_plan_emu"):
        pytest.fail("tests/emu/libhh_emu.so has no gathered reads (make emu)")
    L.hh_blocks_gather_blocks.restype = C.c_int32
    L.hh_blocks_gather_blocks.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.hh_blocks_gather_copy_split.restype = None
    L.hh_blocks_gather_copy_split.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.hh_blocks_gather_plan_emu.restype = C.c_int32
    L.hh_blocks_gather_plan_emu.argtypes = [C.c_void_p] + [C.c_uint64] * 5 + [C.c_void_p, C.c_uint64, C.c_int32] + \
        [C.c_void_p] * 8
    L.hh_blocks_gather_emu_walk.restype = C.c_int64
    L.hh_blocks_gather_emu_walk.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                                               C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                               C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
    return L


# ---------------------------------------------------------------------------
# The host's block rule and the copy's split
# ---------------------------------------------------------------------------
def test_block_count_rule(gemu):
    """nb = ceil(n_syms / block_syms), refused from 2^32 - 1 on and for
    block_syms 0, nothing overflowing."""
    lim = (1 << 32) - 1
    for n_syms, B in [(0, 1), (1, 1), (10, 3), (9, 3), (lim - 1, 1), (lim, 1), (lim + 5, 1), (M64, 1), (M64, 1 << 32),
                      (M64, (1 << 32) + 2), (M64, M64), (M64 - 1, M64), (2 * lim - 3, 2), (2 * lim - 2, 2), (2 * lim - 1, 2),
                      (5, 0), (0, 0)]:
        nb = C.c_uint64(M64)
        ok = gemu.hh_blocks_gather_blocks(n_syms, B, C.byref(nb))
        want = -(-n_syms // B) if B else None
        if want is None or want >= lim:
            assert not ok and nb.value == M64, (n_syms, B)
        else:
            assert ok and nb.value == want, (n_syms, B)


def test_copy_split(gemu):
    """Every destination alignment and every length up to 70: head bytes up
    to the first 16-byte boundary, whole aligned blocks, a tail below 16 --
    together exactly the piece's bytes."""
    for a in range(16):
        for keep in range(71):
            for hi in (0, 1 << 40, M64 - 255):
                dst = hi + a
                h, b = C.c_uint32(77), C.c_uint32(77)
                gemu.hh_blocks_gather_copy_split(dst, keep, C.byref(h), C.byref(b))
                h, b = h.value, b.value
                tail = keep - h - 16 * b
                assert 0 <= h < 16 and 0 <= tail < 16 and h <= keep, (a, keep, h, b)
                assert h == min(keep, -a % 16), (a, keep, h)
                if b:
                    assert (dst + h) % 16 == 0


# ---------------------------------------------------------------------------
# The plan: pieces grouped by block
# ---------------------------------------------------------------------------
def run_gplan(L, reads, n_syms, B, out_bytes, P, index, data_bytes, reverse):
    reads = np.ascontiguousarray(reads, np.uint64).reshape(-1, 3)
    index = np.ascontiguousarray(index, np.uint64).reshape(-1, 4)
    m, nb = reads.shape[0], index.shape[0]
    rstat = np.full(m, 77, np.int32)
    total, T = C.c_uint64(0), C.c_uint32(77)
    cnt, end, first = np.full(nb, 77, np.uint32), np.full(nb, 77, np.uint64), np.full(nb, 77, np.uint32)
    lst = np.full((max(P, 1), 5), 77, np.uint64)
    key = np.full(max(P, 1), 77, np.uint8)
    rc = L.hh_blocks_gather_plan_emu(reads.ctypes.data, m, n_syms, B, out_bytes, P, index.ctypes.data, data_bytes,
                                     int(reverse), rstat.ctypes.data, C.byref(total), cnt.ctypes.data, end.ctypes.data,
                                     first.ctypes.data, C.byref(T), lst.ctypes.data, key.ctypes.data)
    assert rc == 0
    return rstat.tolist(), int(total.value), cnt.tolist(), end.tolist(), first.tolist(), int(T.value), lst, key


def check_gplan(L, reads, n_syms, B, out_bytes, bad_blocks=(), P=None):
    """The grouped plan against test_blocks_read.model(), with the pieces
    placed in slot order and last first."""
    if P is None:
        P = budget(out_bytes, B, len(reads))
    nb = -(-n_syms // B)
    idx, data_bytes = _index(nb, bad_blocks)
    want_stat, _, want_pieces = model(reads, n_syms, B, out_bytes, P, bad_blocks)
    by_block = {}
    for i, b, skip, cap, out_off, ok in want_pieces:
        if ok:
            by_block.setdefault(b, []).append((i, b, skip, cap, out_off))
    lists = []
    for reverse in (False, True):
        stat, total, cnt, end, first, T, lst, key = run_gplan(L, reads, n_syms, B, out_bytes, P, idx, data_bytes, reverse)
        assert stat == want_stat, (reads, stat, want_stat)
        assert total == len(want_pieces) <= P
        assert key[:total].tolist() == [0 if p[5] else INVALID for p in want_pieces]
        assert T == len(by_block) <= min(nb, P)
        pos = 0
        for b in range(nb):
            mine = by_block.get(b, [])
            assert cnt[b] == len(mine) and first[b] == pos, (b, cnt[b], first[b], pos)
            assert end[b] == max((p[2] + p[3] for p in mine), default=0)
            got = [tuple(r) for r in lst[pos: pos + cnt[b]].tolist()]
            assert sorted(got) == sorted(mine), (b, got, mine)           # as a set: exactly the block's valid pieces
            lists.append(got)
            pos += cnt[b]
        assert pos == sum(len(v) for v in by_block.values())
    half = len(lists) // 2
    return want_stat, want_pieces, any(a != b for a, b in zip(lists[:half], lists[half:]))


@pytest.mark.parametrize("B", [1, 7, 4096])
def test_plan_at_block_edges(gemu, B):
    """test_blocks_read.py::test_read_rules_at_block_edges' reads, grouped;
    with two bad index entries as well."""
    n_syms = 3 * B + (B + 1) // 2
    edges = sorted({e + d for e in (0, B, 2 * B, 3 * B, n_syms) for d in (-1, 0, 1) if 0 <= e + d <= n_syms + 1})
    reads, off = [], 3
    for a in edges:
        for b in edges:
            if a <= b:
                reads.append((a, b - a, off))
                off += b - a
    reads += [(n_syms, 0, off), (n_syms + 1, 0, off), (0, 0, off), (0, 0, off + 1), (0, 1, off), (n_syms - 1, 1, off - 1)]
    stat, pieces, differ = check_gplan(gemu, reads, n_syms, B, off)
    assert stat.count(ERR_ARG) >= len(edges) and stat.count(0) > len(edges) and differ
    check_gplan(gemu, reads, n_syms, B, off, bad_blocks=(1, 3))


def test_plan_budget_overflow(gemu):
    """test_blocks_read.py::test_budget's overlapping reads: the budget
    reached, exceeded by one and by a whole read; the reads past it have no
    piece in any block's list."""
    n_syms, B, out_bytes = 30, 7, 14
    stat, pieces, _ = check_gplan(gemu, [(3, 14, 0), (6, 14, 0)], n_syms, B, out_bytes)
    assert stat == [0, 0] and len(pieces) == 6
    stat, pieces, _ = check_gplan(gemu, [(3, 14, 0), (6, 14, 0), (5, 14, 0), (0, 0, 0), (0, 1, 0)], n_syms, B, out_bytes, P=8)
    assert stat == [0, 0, ERR_ARG, 0, ERR_ARG] and len(pieces) == 6
    reads = [(3, 14, 0), (6, 14, 0), (0, 8, 0), (0, 1, 0)]
    stat, pieces, _ = check_gplan(gemu, reads, n_syms, B, out_bytes, P=8)
    assert stat == [0, 0, 0, ERR_ARG] and len(pieces) == 8
    stat, pieces, _ = check_gplan(gemu, reads, n_syms, B, out_bytes, P=9)
    assert stat == [0, 0, 0, 0] and len(pieces) == 9


def test_plan_random(gemu):
    """test_blocks_read.py::test_plan_random's 2000 cases (same generator,
    same seed), grouped: bad blocks, budgets below the formula's, empty and
    rangeless reads."""
    rng = np.random.default_rng(2000)
    seen = {"bad": 0, "budget": 0, "shared": 0, "order": 0}
    for _ in range(2000):
        B = int(rng.choice([1, 2, 3, 7, 16]))
        n_syms = int(rng.integers(0, 6 * B + 2))
        out_bytes = int(rng.integers(0, 3 * B + 8))
        m = int(rng.integers(1, 7))
        reads = []
        for _ in range(m):
            s = int(rng.integers(0, n_syms + 2))
            l = int(rng.integers(0, max(1, min(n_syms - s, out_bytes) + 2))) if rng.random() < 0.85 else 0
            d = int(rng.integers(0, max(1, out_bytes - l + 2)))
            reads.append((s, l, d))
        nb = -(-n_syms // B)
        bad = tuple(int(b) for b in np.flatnonzero(rng.random(nb) < 0.15))
        P = budget(out_bytes, B, m)
        if rng.random() < 0.33:
            P = int(rng.integers(0, P))
        stat, pieces, differ = check_gplan(gemu, reads, n_syms, B, out_bytes, bad_blocks=bad, P=P)
        blocks = [p[1] for p in pieces if p[5]]
        seen["bad"] += any(not p[5] for p in pieces)
        seen["budget"] += ERR_ARG in stat and len(pieces) > 0
        seen["shared"] += len(blocks) != len(set(blocks))
        seen["order"] += differ
    assert all(v >= 100 for v in seen.values()), seen


# ---------------------------------------------------------------------------
# The merged walk
# ---------------------------------------------------------------------------
def run_walk(L, c, data, bits, pieces, out, W, S, K):
    """One block (data_off 0, bits) walked once for pieces (out_off, cap,
    skip): (rc, len, status, rounds walked, rounds emitted)."""
    iz = np.ascontiguousarray(c.izero, np.int32)
    io = np.ascontiguousarray(c.ione, np.int32)
    sy = np.ascontiguousarray(c.sym, np.uint8)
    data = np.ascontiguousarray(data, np.uint8)
    pieces = np.ascontiguousarray(pieces, np.uint64).reshape(-1, 3)
    n = pieces.shape[0]
    ln = np.zeros(max(n, 1), np.uint64)
    status = np.full(max(n, 1), 77, np.int32)
    rounds, emitted, rb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.hh_blocks_gather_emu_walk(iz.ctypes.data, io.ctypes.data, sy.ctypes.data, len(iz), data.ctypes.data, data.size,
                                     0, bits, pieces.ctypes.data, n, S, K, W, out.ctypes.data, out.size, ln.ctypes.data,
                                     status.ctypes.data, C.byref(rounds), C.byref(emitted), C.byref(rb))
    return int(rc), ln[:n].tolist(), status[:n].tolist(), int(rounds.value), int(emitted.value)


def piece_lists(cs, end):
    """Piece lists (skip, cap) of a block of `end` symbols whose rounds end at
    the symbol counts cs: the first and the last byte of every round, windows
    across every boundary, windows inside one round (one and several), empty
    windows, the whole block; alone and together."""
    lo = [0] + list(cs)
    hi = list(cs) + [end]
    firsts = [(a, 1) for a in lo]
    lasts = [(b - 1, 1) for b in hi]
    straddle = [(c - 1, 2) for c in cs] + [(cs[0] - 3, cs[1] - cs[0] + 6)]
    inside = [(a + (b - a) // 3, (b - a) // 3) for a, b in zip(lo, hi)]
    several = [(lo[1] + k * 7, 5) for k in range(6)] + [(lo[1] + 3, 20)]           # overlapping sources are fine
    empty = [(0, 0), (cs[0], 0), (end, 0)]
    lists = [[w] for w in block_windows(cs, end)]                                  # each of the single-piece windows
    lists += [firsts, lasts, straddle, inside, several, [(0, end)] + inside, firsts[:2] + lasts[:1],
              several + empty[:1], inside[:1] + straddle[:1],
              firsts + lasts + straddle + inside + several + [(0, end)]]
    return lists


WALK_NAMES = EC.CODE_NAMES + E.SHAPE_NAMES


@pytest.mark.parametrize("W", [1, 2, 16])
@pytest.mark.parametrize("name", WALK_NAMES)
def test_merged_walk(gemu, name, W):
    """A block of three rounds + one region + 1 bit, as
    test_blocks_read.py::test_windowed_rounds builds it, at the library's S
    and K.  For every list of piece_lists the merged walk gives the bytes,
    lengths and statuses of hh_blocks_read_emu_decode run piece by piece (and
    nothing outside the windows), in the rounds of the largest skip + cap --
    not the block's -- emitting only the rounds a piece has bytes in."""
    S, K = GEO[name][:2]
    c = E.any_code(name)
    rb = 64 * W * S
    data, total_bits, _ = E.stream(name, S, 49)
    bits = 3 * rb + S + 1
    assert bits <= total_bits
    ref = EC.oracle_prefix(c, data, bits)
    end = len(ref)
    cs = round_counts(c, data, bits, rb, ref)
    assert len(cs) == 3 and 0 < cs[0] < cs[1] < cs[2] < end and cs[0] > 8 and cs[1] - cs[0] > 64
    for wins in piece_lists(cs, end):
        offs, off = [], 1
        for k, (skip, cap) in enumerate(wins):
            offs.append(off)
            off += cap + (k % 3 == 0)                            # some destinations touch, some leave a byte
        want_out = np.full(off + 64, 0xAB, np.uint8)
        full = [[0, bits, o, cap, skip] for o, (skip, cap) in zip(offs, wins)]
        rc, wlen, wstat, wrounds, _ = run_decode(gemu, c, data, full, want_out, W, S, K)
        assert rc == 0
        out = np.full(off + 64, 0xAB, np.uint8)
        rc, ln, status, rounds, emitted = run_walk(gemu, c, data, bits, [[o, cap, skip] for o, (skip, cap) in zip(offs, wins)],
                                                   out, W, S, K)
        assert rc == 0
        assert ln == wlen == [cap for _, cap in wins] and status == wstat and not any(status)
        assert np.array_equal(out, want_out)
        for o, (skip, cap) in zip(offs, wins):
            assert np.array_equal(out[o: o + cap], ref[skip: skip + cap])
        far = max((s + n for s, n in wins if n), default=0)
        assert rounds == max(wrounds) == (rounds_for(cs, far - 1, 1) if far else 0)
        in_round = lambda r: any(max(s, ([0] + cs)[r]) < min(s + n, (cs + [end])[r]) for s, n in wins)
        assert emitted == sum(in_round(r) for r in range(rounds))


@pytest.mark.parametrize("name,W", [("kjv", 2), ("byte256", 1), ("caterpillar40", 2), ("lattice5", 16), ("random12", 2)])
def test_delivered_bytes_in_a_short_block(gemu, name, W):
    """The index says a little over half the block's bits.  Of several pieces
    some lie before the stream's end (full), one across it (partial), some
    past it (empty): lengths and statuses by the delivered-bytes rule and
    equal to the piece-by-piece decode's; the bytes the stream holds are
    delivered and nothing past them."""
    S, K = GEO[name][:2]
    c = E.any_code(name)
    rb = 64 * W * S
    data, total_bits, _ = E.stream(name, S, 49)
    bits = rb + rb // 2 + 5                                      # (ends inside round 1, inside a code or not)
    half = EC.oracle_prefix(c, data, bits)
    h = len(half)
    wins = [(0, 10), (h - 40, 30), (h - 10, 25), (h + 3, 9), (h - 1, 1), (h, 1), (5, h + 100), (h + 200, 50), (h // 2, 3)]
    offs, off = [], 2
    for skip, cap in wins:
        offs.append(off)
        off += cap
    want_out = np.full(off + 64, 0xAB, np.uint8)
    rc, wlen, wstat, wrounds, _ = run_decode(gemu, c, data, [[0, bits, o, cap, skip] for o, (skip, cap) in zip(offs, wins)],
                                             want_out, W, S, K)
    assert rc == 0
    out = np.full(off + 64, 0xAB, np.uint8)
    rc, ln, status, rounds, emitted = run_walk(gemu, c, data, bits, [[o, cap, skip] for o, (skip, cap) in zip(offs, wins)],
                                               out, W, S, K)
    assert rc == 0 and rounds == 2 == emitted
    assert ln == [max(0, min(h, s + n) - s) for s, n in wins] == wlen
    assert status == [0 if s + n <= h else ERR_FORMAT for s, n in wins] == wstat
    assert status.count(0) == 4 and ln[2] == 10 and ln[3] == 0 and ln[6] == h - 5
    assert np.array_equal(out, want_out)
    for o, (s, n), got in zip(offs, wins, ln):
        assert np.array_equal(out[o: o + got], half[s: s + got]) and (out[o + got: o + n] == 0xAB).all()
