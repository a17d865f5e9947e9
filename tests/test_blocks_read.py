"""Range reads over a block-coded buffer (hh_decode_blocks_read) on the host:
the emulator (tests/emu/hh_blocks_read_emu.cpp) compiles the very rules the
kernels run -- hb_window of csrc/hh_batch_algo.h, the read rules of
csrc/hh_batch_read_algo.h -- and runs the plan read by read and k_batch's
windowed rounds lane by lane.  The read rules keep a bad read from becoming
an address, so their overflow corners are checked here and never sent to a
GPU.  tests/test_gpu_blocks_read.py runs the kernels."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import edge_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libhh_emu.so")
M64 = (1 << 64) - 1
PAD = 64                    # HH_PAYLOAD_PAD
RB = 64 * 16 * 128          # a round's bits at W = 16, S = 128
ERR_ARG, ERR_FORMAT = -1, -3
INVALID = 0x80
NONE = M64


@pytest.fixture(scope="module")
def remu():
    if not os.path.exists(EMU):
        pytest.skip("tests/emu/libhh_emu.so not built (make emu)")
    L = C.CDLL(EMU)
    L.hh_blocks_read_window.restype = C.c_uint32
    L.hh_blocks_read_window.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.hh_blocks_read_ok.restype = C.c_int32
    L.hh_blocks_read_ok.argtypes = [C.c_uint64] * 5
    L.hh_blocks_read_budget.restype = C.c_int32
    L.hh_blocks_read_budget.argtypes = [C.c_uint64] * 3 + [C.POINTER(C.c_uint64)]
    L.hh_blocks_read_plan_emu.restype = C.c_int32
    L.hh_blocks_read_plan_emu.argtypes = [C.c_void_p] + [C.c_uint64] * 5 + [C.c_void_p, C.c_uint64, C.c_uint64] + \
        [C.c_void_p] * 4
    L.hh_blocks_read_emu_decode.restype = C.c_int64
    L.hh_blocks_read_emu_decode.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


# ---------------------------------------------------------------------------
# hb_window
# ---------------------------------------------------------------------------
def window(base, n, skip, cap):
    """(keep, from) in Python's unbounded integers: the round's bytes
    [base, base + n) that lie in [skip, skip + cap)."""
    lo, hi = max(base, skip), min(base + n, skip + cap)
    return (hi - lo, lo - base) if hi > lo else (0, 0)


def _window(L, base, n, skip, cap):
    f = C.c_uint32(77)
    k = L.hh_blocks_read_window(base, n, skip, cap, C.byref(f))
    return int(k), int(f.value)


def test_window_small_exhaustive(remu):
    """Every base, n, skip, cap up to 12."""
    for base, n, skip, cap in itertools.product(range(13), repeat=4):
        assert _window(remu, base, n, skip, cap) == window(base, n, skip, cap), (base, n, skip, cap)


def test_window_large(remu):
    """Around 2^63 and 2^64 - 1: base + n and skip + cap pass 2^64 and the
    rule forms neither sum."""
    big = [0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 5, M64 - 1, M64]
    ns = [0, 1, 5, (1 << 32) - 1]
    for base, n, skip, cap in itertools.product(big, ns, big, big):
        assert _window(remu, base, n, skip, cap) == window(base, n, skip, cap), (base, n, skip, cap)
    # with no skip it is hb_clip
    for base, n, cap in itertools.product(big, ns, big):
        assert _window(remu, base, n, 0, cap) == (max(0, min(base + n, cap) - base), 0)


# ---------------------------------------------------------------------------
# The read rules and the plan
# ---------------------------------------------------------------------------
def budget(out_bytes, B, m):
    P = out_bytes // B + 2 * m
    return P if P < (1 << 32) - 1 else None


def _budget(L, out_bytes, B, m):
    P = C.c_uint64(M64)
    ok = L.hh_blocks_read_budget(out_bytes, B, m, C.byref(P))
    assert ok or P.value == M64
    return int(P.value) if ok else None


def model(reads, n_syms, B, out_bytes, P, bad_blocks=()):
    """The plan in Python integers: (status per read, first slot per read,
    the pieces (owner, block, skip, cap, out_off, valid) in slot order)."""
    stat, first, pieces = [], [], []
    carry, full = 0, False
    for i, (s, l, d) in enumerate(reads):
        ok = s + l <= n_syms and d + l <= out_bytes
        c = (s + l - 1) // B - s // B + 1 if ok and l else 0
        first.append(carry)
        if c and carry + c > P:
            ok, full = False, True
        elif not full:
            for b in range(s // B, s // B + c):
                lo, hi = max(s, b * B), min(s + l, (b + 1) * B)
                pieces.append((i, b, lo - b * B, hi - lo, d + lo - s, b not in bad_blocks))
        carry += c
        stat.append(0 if ok else ERR_ARG)
    return stat, first, pieces


def run_plan(L, reads, n_syms, B, out_bytes, P, index, data_bytes):
    reads = np.ascontiguousarray(reads, np.uint64).reshape(-1, 3)
    index = np.ascontiguousarray(index, np.uint64).reshape(-1, 4)
    m = reads.shape[0]
    rstat = np.full(m, 77, np.int32)
    first = np.zeros(m, np.uint64)
    total = C.c_uint64(0)
    piece = np.full((P, 8), 77, np.uint64)
    rc = L.hh_blocks_read_plan_emu(reads.ctypes.data, m, n_syms, B, out_bytes, P, index.ctypes.data, data_bytes, RB,
                                   rstat.ctypes.data, first.ctypes.data, C.byref(total), piece.ctypes.data)
    assert rc == 0
    return rstat.tolist(), first.tolist(), int(total.value), piece


def _index(nb, bad_blocks=()):
    """nb entries of 8 bits each, 4 bytes apart; the bad ones alternately off
    a 4-byte boundary and reaching past data_bytes."""
    idx = np.zeros((nb, 4), np.uint64)
    idx[:, 0] = 4 * np.arange(nb)
    idx[:, 1] = 8 + np.arange(nb) % 5
    data_bytes = 4 * nb + 4 + PAD
    for k, b in enumerate(sorted(bad_blocks)):
        if k % 2:
            idx[b, 0] = data_bytes - PAD
        else:
            idx[b, 0] += 1
    return idx, data_bytes


def check_plan(L, reads, n_syms, B, out_bytes, bad_blocks=(), P=None):
    if P is None:
        P = _budget(L, out_bytes, B, len(reads))
        assert P == budget(out_bytes, B, len(reads))
    idx, data_bytes = _index(-(-n_syms // B), bad_blocks)
    want_stat, want_first, want_pieces = model(reads, n_syms, B, out_bytes, P, bad_blocks)
    stat, first, total, piece = run_plan(L, reads, n_syms, B, out_bytes, P, idx, data_bytes)
    assert stat == want_stat, (reads, n_syms, B, out_bytes, stat, want_stat)
    assert total == len(want_pieces) <= P
    for s, (i, b, skip, cap, out_off, ok) in enumerate(want_pieces):
        assert piece[s, :5].tolist() == [i, b, skip, cap, out_off], (s, reads[i], piece[s])
        assert first[i] <= s
        if ok:
            assert piece[s, 5:].tolist() == [idx[b, 0], idx[b, 1], 1]
        else:
            assert piece[s, 5:].tolist() == [0, 0, INVALID]          # (never an address)
        # a piece lies inside its read's destination and inside its block
        rs, rl, rd = reads[i]
        assert rd <= out_off and out_off + cap <= rd + rl and 0 < cap and skip + cap <= min(B, n_syms - b * B)
    for s in range(total, P):
        assert piece[s].tolist() == [NONE, 0, 0, 0, 0, 0, 0, 0]       # padding: the empty descriptor, bin 0
    for i, (st, (s, l, d)) in enumerate(zip(want_stat, reads)):
        if st == 0 and l:
            assert sum(p[3] for p in want_pieces if p[0] == i) == l
    return want_stat, want_pieces


@pytest.mark.parametrize("B", [1, 7, 4096])
def test_read_rules_at_block_edges(remu, B):
    """Reads that start or end at a block edge or one byte either side of
    it, empty reads, reads ending at n_syms and one past it; destinations
    packed back to back (disjoint: the budget holds)."""
    n_syms = 3 * B + (B + 1) // 2
    edges = sorted({e + d for e in (0, B, 2 * B, 3 * B, n_syms) for d in (-1, 0, 1) if 0 <= e + d <= n_syms + 1})
    reads, off = [], 3
    for a in edges:
        for b in edges:
            if a <= b:
                reads.append((a, b - a, off))
                off += b - a
    reads += [(n_syms, 0, off), (n_syms + 1, 0, off), (0, 0, off), (0, 0, off + 1), (0, 1, off), (n_syms - 1, 1, off - 1)]
    out_bytes = off
    stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes)
    assert stat.count(ERR_ARG) >= len(edges) and stat.count(0) > len(edges)
    for (s, l, d), st in zip(reads, stat):
        assert (st == 0) == (s + l <= n_syms and d + l <= out_bytes)
    # the same with two index entries that break a rule
    check_plan(remu, reads, n_syms, B, out_bytes, bad_blocks=(1, 3))


def test_read_rule_wraps(remu):
    """src_off + len and dst_off + len past 2^64, in every combination with
    sizes at 0, small and 2^64 - 1."""
    vals = [0, 1, 100, (1 << 63) - 1, 1 << 63, M64 - 100, M64 - 1, M64]
    for s, l, d in itertools.product(vals, repeat=3):
        for n_syms, out_bytes in ((100, 100), (M64, 100), (100, M64), (M64, M64), (0, 0), (1 << 63, M64 - 1)):
            want = s + l <= n_syms and d + l <= out_bytes
            assert bool(remu.hh_blocks_read_ok(s, l, d, n_syms, out_bytes)) == want, (s, l, d, n_syms, out_bytes)
    # a wrapped read among good ones gets no piece
    reads = [(0, 10, 0), (M64, 2, 0), (5, M64, 0), (0, 5, M64 - 2), (10, 4, 10), (M64 - 3, 4, 14)]
    stat, pieces = check_plan(remu, reads, 14, 7, 14)
    assert stat == [0, ERR_ARG, ERR_ARG, ERR_ARG, 0, ERR_ARG] and {p[0] for p in pieces} == {0, 4}


def test_budget(remu):
    """P = out_bytes / block_syms + 2 m, refused from 2^32 - 1 on, none of it
    overflowing; and the plan with P exactly reached and exceeded by one
    (destinations overlap: disjoint ones cannot get there)."""
    lim = (1 << 32) - 1
    cases = [(1 << 40, 1, 1), (lim - 3, 1, 1), (lim - 2, 1, 1), (lim - 4, 1, 1), (0, 1, lim // 2), (0, 1, lim // 2 - 1),
             (1, 1, lim // 2 - 1), (M64, 1 << 32, 1), (M64, 1 << 33, 1), (M64, M64, 1), (M64, 1, 1), (0, 7, 1 << 63),
             (0, 7, M64), (0, 7, 1 << 31), (100, 7, 3), (0, 4096, 0), (14, 7, 2)]
    for out_bytes, B, m in cases:
        assert _budget(remu, out_bytes, B, m) == budget(out_bytes, B, m), (out_bytes, B, m)
    assert _budget(remu, 1 << 40, 1, 1) is None and _budget(remu, lim - 4, 1, 1) == lim - 2
    assert _budget(remu, 100, 0, 1) is None
    # two reads of three blocks each into the same 14 bytes: 6 pieces, P = 2 + 2 * 2
    n_syms, B, out_bytes = 30, 7, 14
    reads = [(3, 14, 0), (6, 14, 0)]
    stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes)
    assert stat == [0, 0] and len(pieces) == 6 == budget(out_bytes, B, 2)
    # three of them: 9 pieces for P = 8 -- the third gets none; an empty and a small read after it
    reads = [(3, 14, 0), (6, 14, 0), (5, 14, 0), (0, 0, 0), (0, 1, 0)]
    stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes, P=8)
    assert stat == [0, 0, ERR_ARG, 0, ERR_ARG] and len(pieces) == 6
    # exceeded by exactly one
    reads = [(3, 14, 0), (6, 14, 0), (0, 8, 0), (0, 1, 0)]
    assert budget(out_bytes, B, 4) == 10
    stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes, P=8)
    assert stat == [0, 0, 0, ERR_ARG] and len(pieces) == 8
    stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes, P=9)
    assert stat == [0, 0, 0, 0] and len(pieces) == 9


def test_plan_random(remu):
    """2000 small cases: random reads, some out of range at either end, some
    empty, destinations anywhere (overlaps exhaust the budget), index entries
    that break a rule.  Every rule fires at least a hundred times."""
    rng = np.random.default_rng(2000)
    fired = {"src": 0, "dst": 0, "empty": 0, "budget": 0, "entry": 0, "cross": 0, "ok": 0}
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
        # (disjoint destinations never exhaust the budget and overlapping ones seldom: a third of the
        # cases run the plan with fewer slots than the budget)
        P = budget(out_bytes, B, m)
        if rng.random() < 0.33:
            P = int(rng.integers(0, P))
        stat, pieces = check_plan(remu, reads, n_syms, B, out_bytes, bad_blocks=bad, P=P)
        carry = 0
        for (s, l, d), st in zip(reads, stat):
            src, dst = s + l <= n_syms, d + l <= out_bytes
            fired["src"] += not src
            fired["dst"] += not dst
            fired["empty"] += src and dst and l == 0
            c = (s + l - 1) // B - s // B + 1 if src and dst and l else 0
            fired["budget"] += bool(c) and carry + c > P
            fired["cross"] += st == 0 and c > 1
            fired["ok"] += st == 0 and c > 0
            carry += c
        fired["entry"] += sum(not p[5] for p in pieces)
    assert all(v >= 100 for v in fired.values()), fired


# ---------------------------------------------------------------------------
# Windowed rounds
# ---------------------------------------------------------------------------
def run_decode(L, c, data, pieces, out, W):
    iz = np.ascontiguousarray(c.izero, np.int32)
    io = np.ascontiguousarray(c.ione, np.int32)
    sy = np.ascontiguousarray(c.sym, np.uint8)
    data = np.ascontiguousarray(data, np.uint8)
    pieces = np.ascontiguousarray(pieces, np.uint64).reshape(-1, 5)
    n = pieces.shape[0]
    ln = np.zeros(n, np.uint64)
    status = np.full(n, 77, np.int32)
    rounds = np.zeros(n, np.uint64)
    rb = C.c_uint64(0)
    rc = L.hh_blocks_read_emu_decode(iz.ctypes.data, io.ctypes.data, sy.ctypes.data, len(iz), data.ctypes.data, data.size,
                                     pieces.ctypes.data, n, 0, 0, W, out.ctypes.data, out.size, ln.ctypes.data,
                                     status.ctypes.data, rounds.ctypes.data, C.byref(rb))
    return int(rc), ln.tolist(), status.tolist(), rounds.tolist(), int(rb.value)


def round_counts(c, data, bits, rb, ref):
    """The symbols complete at each round boundary below `bits` (a code that
    straddles the boundary belongs to the round it ends in): the oracle's
    prefix decode, less the tail rule's symbol when the boundary cuts a code."""
    L = E._lengths(c.izero, c.ione, c.sym)
    tab = np.full(256, 1 << 40, np.int64)                       # (a tail-rule byte ends no code)
    tab[list(L)] = list(L.values())
    cum = np.cumsum(tab[ref])
    out = []
    for k in range(1, (bits - 1) // rb + 1):
        n = int(np.searchsorted(cum, k * rb, side="right"))
        p = E.oracle_prefix(c, data, k * rb)
        assert len(p) == n + (n == 0 or cum[n - 1] < k * rb) or len(p) == n
        assert np.array_equal(p[:n], ref[:n])
        out.append(n)
    return out


def block_windows(cs, end):
    """(skip, cap) for the symbol counts cs at the round boundaries of a block
    of `end` symbols: [0,c), [c-1,c+1), [c,c+1), [c,end), the empty window
    and the whole block."""
    w = [(0, 0), (0, end), (end, 0)]
    for c in cs:
        w += [(0, c), (c - 1, 2), (c, 1), (c, end - c)]
    return w


def rounds_for(cs, skip, cap):
    """The index of the round that holds the window's last byte, plus one."""
    return 0 if cap == 0 else sum(c <= skip + cap - 1 for c in cs) + 1


@pytest.mark.parametrize("W", [1, 2, 16])
@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_windowed_rounds(remu, name, W):
    """A block of a little over three rounds; every window of block_windows
    gives the oracle's slice, nothing outside it is written, and the rounds
    walked are those up to the window's last byte: the early stop."""
    c = E.code(name)
    out0 = np.zeros(16, np.uint8)
    rc, _, _, _, rb = run_decode(remu, c, np.zeros(256, np.uint8), [[0, 8, 0, 1, 0]], out0, W)
    assert rc == 0 and rb % (64 * W * 32) == 0
    S = rb // (64 * W)
    data, total_bits, _ = E.stream(name, S, 49)
    bits = 3 * rb + S + 1
    assert bits <= total_bits
    ref = E.oracle_prefix(c, data, bits)
    end = len(ref)
    cs = round_counts(c, data, bits, rb, ref)
    assert len(cs) == 3 and 0 < cs[0] < cs[1] < cs[2] < end
    wins = block_windows(cs, end)
    pieces, off = [], 1
    for skip, cap in wins:
        pieces.append([0, bits, off, cap, skip])
        off += cap
    out = np.full(off + 64, 0xAB, np.uint8)
    rc, ln, status, rounds, _ = run_decode(remu, c, data, pieces, out, W)
    assert rc == 0 and not any(status), status
    want = np.full(out.size, 0xAB, np.uint8)
    for (_, _, o, cap, skip), n, r in zip(pieces, ln, rounds):
        assert n == cap and r == rounds_for(cs, skip, cap), (skip, cap, n, r, cs)
        want[o: o + cap] = ref[skip: skip + cap]
    assert np.array_equal(out, want)
    # a window past the stream's end: HH_ERR_FORMAT, the bytes there are delivered
    out = np.full(64, 0xAB, np.uint8)
    rc, ln, status, rounds, _ = run_decode(remu, c, data, [[0, bits, 8, 20, end - 5]], out, W)
    assert rc == 0 and status == [ERR_FORMAT] and ln == [5] and rounds == [4]
    assert np.array_equal(out[8:13], ref[end - 5:]) and (out[:8] == 0xAB).all() and (out[13:] == 0xAB).all()
