"""The batched decode's round rules over the tables the library really uses:
shape_cases' family (trees picked for the geometry hh_decoder_set_tree
derives from them) and every emission step the builder can be asked for,
through the emulators of tests/test_emu_batch.py and tests/test_blocks_read.py
(whose files stay as they are: the two test bodies this file needs with K as a
parameter are restated here).

Those two files call the emulator with K = 0, the builder's default of 6, on
trees whose regions are 256 or 224 bits: a remainder step of 4 or 2 bits
behind 6-bit steps and nothing else.  Here hb_region walks `er` tables of r
in {1, 2, 3, 4, 6} behind steps of 4 .. 7 bits over regions of 160, 192,
224 and 256 bits, hb_guess takes heads that are multiples of each K, and
kjv's K = 7 tables -- the ones the library uses for it -- are run at all.
tests/test_gpu_batch_shapes.py decodes the same shapes on the GPU at the
geometry Decoder.geometry() reports: a shape that fails here is wrong in the
rules or the tables, one that fails only there in k_batch or its launch."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as EC
import shape_cases as E
from test_blocks_read import ERR_FORMAT, block_windows, remu, round_counts, rounds_for  # noqa: F401  (remu: a fixture)
from test_emu_batch import GUARD, batch_cuts, bemu, run_bemu  # noqa: F401  (bemu: a fixture)

_REFS = {}                 # (code, S, bits) -> the oracle's decode of E.stream(code, S, 49)'s first bits


def _ref(name, S, data, bits):
    r = _REFS.get((name, S, bits))
    if r is None:
        r = _REFS[(name, S, bits)] = EC.oracle_prefix(E.any_code(name), data, bits)
    return r


def breakpoints(bemu, name, W, K, S):
    """test_emu_batch.py::test_batch_breakpoints' body for a code or a shape,
    the emission step asked for and regions of S bits: one batch of every cut
    of batch_cuts, all prefixes of one stream, the outputs packed back to
    back from out_off 1 with each capacity exactly the oracle's length --
    every stream's bytes and length the oracle's, every status 0, the byte
    before the first output and those after the last untouched.  Returns the
    emulator's stats."""
    c = E.any_code(name)
    data, bits, _ = E.stream(name, S, 49)
    cuts = batch_cuts(S, W, c.tree().info()["maxlen"], bits)
    assert cuts[-1] == 3 * W * 64 * S + S + 1 and W * 64 * S in cuts
    refs = [_ref(name, S, data, b) for b in cuts]
    items, off = [], 1
    for b, r in zip(cuts, refs):
        items.append([0, b, off, len(r)])
        off += len(r)
    out = np.full(off + GUARD, 0xAB, np.uint8)
    rc, out_len, status, st = run_bemu(bemu, c.izero, c.ione, c.sym, data, items, out, W, S=S, K=K)
    assert rc == 0 and not status.any(), (rc, status, st)
    for (_, b, o, n), r, got in zip(items, refs, out_len):
        assert got == n and np.array_equal(out[o: o + n], r), (b, divmod(b, 64 * S), got, n)
    assert out[0] == 0xAB and (out[off:] == 0xAB).all()
    return st


def run_decode(L, c, data, pieces, out, W, S, K):
    """test_blocks_read.py's run_decode with the region bits and the emission
    step asked for."""
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
                                     pieces.ctypes.data, n, S, K, W, out.ctypes.data, out.size, ln.ctypes.data,
                                     status.ctypes.data, rounds.ctypes.data, C.byref(rb))
    return int(rc), ln.tolist(), status.tolist(), rounds.tolist(), int(rb.value)


KS = (4, 5, 6, 7)
GEO = {**E.CODE_GEOMETRY, **E.SHAPE_GEOMETRY}
# every shape at every K asked and W in {1, 2}, and at 16 waves at the K the library picks for it; the
# codes of CODE_NAMES at the two steps other than the default that the library picks among them (7: kjv,
# fixed2; 5: byte256), and at 16 waves at their own
GRID = [(n, K, W) for n in E.SHAPE_NAMES for K in KS for W in (1, 2)] + \
       [(n, E.SHAPE_GEOMETRY[n][1], 16) for n in E.SHAPE_NAMES] + \
       [(n, K, 2) for n in E.CODE_NAMES for K in (7, 5)] + \
       [(n, E.CODE_GEOMETRY[n][1], 16) for n in E.CODE_NAMES if E.CODE_GEOMETRY[n][1] != 6]


def built_k(c, K):
    """The step hh_fsm_build gives when asked for K: a code with a 1-bit
    symbol takes 4 (a step may complete no more than four symbols), more than
    127 states at most 6 (the entry's row field)."""
    if c.tree().info()["minlen"] < 2:
        return 4
    return 6 if K == 7 and int((np.asarray(c.izero) >= 0).sum()) > 127 else K


def test_shape_family():
    """The shapes are what their names say: states, code lengths, the
    distribution; the existing names' streams keep their seeds."""
    want = {"complete5": (31, {5}), "complete7": (127, {7}), "complete8": (255, {8}), "lattice3": (14, {3, 6}),
            "lattice5": (62, {5, 10}), "lattice6": (126, {6, 12}), "split7": (128, {7, 8}),
            "caterpillar64": (64, set(range(1, 65)))}
    assert set(E.SHAPE_NAMES) == set(E.SHAPE_GEOMETRY) and not set(E.SHAPE_NAMES) & set(E.CODE_NAMES)
    for k, name in enumerate(E.CODE_NAMES):
        assert E.name_index(name) == k and E.any_code(name) is EC.code(name)
        assert E.stream(name, 256, 3) is EC.stream(name, 256, 3)
    for name in E.SHAPE_NAMES:
        c = E.shape(name)
        iz, io = np.asarray(c.izero), np.asarray(c.ione)
        assert ((iz >= 0) == (io >= 0)).all()
        ns = int((iz >= 0).sum())
        L = E._lengths(c.izero, c.ione, c.sym)
        assert ns == E.SHAPE_GEOMETRY[name][6] and len(L) == ns + 1, (name, ns, len(L))     # (distinct leaf symbols)
        if name in want:
            assert (ns, set(L.values())) == want[name], name
        info = c.tree().info()
        assert info["minlen"] == min(L.values()) and info["maxlen"] == max(L.values())
        syms, p = c.probs
        assert syms.tolist() == sorted(L) and np.array_equal(p, [2.0 ** -L[int(s)] for s in syms])
        assert c.complete == (len(set(L.values())) == 1) and c.flags == (E.FLAG_NO_FIXED if c.complete else 0)
        assert np.asarray(c.sym)[iz >= 0].all()                  # a cut inside a code shows: the tail rule's byte
    assert E.shape("lattice5").tree().info()["len_gcd"] == 5


@pytest.mark.parametrize("name,K,W", GRID)
def test_batch_breakpoints_at_k(bemu, name, K, W):
    """test_emu_batch.py::test_batch_breakpoints (every batch_cuts prefix,
    outputs packed from offset 1 with exact capacities, 0xAB around, bytes and
    lengths the oracle's chain decode) with the emission step asked for, at
    the region bits the library uses (for fixed1 and fixed2 those are 64 and
    128, not the emulator's default of 256: set_tree shrinks a fixed-length
    code's regions to the single-stream emission's staging); the step the
    builder reports is the one its rules give, and at the library's own K the
    head is the library's."""
    c = E.any_code(name)
    S, K_lib, _, _, G_lib = GEO[name][:5]
    st = breakpoints(bemu, name, W, K, S)
    assert st[0] == S and st[2] == built_k(c, K), (st, S, K)
    assert st[1] % st[2] == 0 and st[1] <= S
    if st[2] == K_lib:
        assert st[1] == G_lib, st


@pytest.mark.parametrize("name", E.SHAPE_NAMES)
def test_windowed_rounds_of_shapes(remu, name):
    """test_blocks_read.py::test_windowed_rounds for the shapes, at the S and
    K the library picks and W = 2: a block of a little over three rounds;
    every window of block_windows gives the oracle's slice, nothing outside it
    is written, and the rounds walked are those up to the window's last byte;
    a window past the stream's end is HH_ERR_FORMAT with the bytes there
    delivered."""
    S, K = E.SHAPE_GEOMETRY[name][:2]
    W = 2
    c = E.shape(name)
    rc, _, _, _, rb = run_decode(remu, c, np.zeros(256, np.uint8), [[0, 8, 0, 1, 0]], np.zeros(16, np.uint8), W, 0, K)
    assert rc == 0 and rb == 64 * W * S                          # (the emulator's default regions are the library's)
    data, total_bits, _ = E.stream(name, S, 49)
    bits = 3 * rb + S + 1
    assert bits <= total_bits
    ref = EC.oracle_prefix(c, data, bits)
    end = len(ref)
    cs = round_counts(c, data, bits, rb, ref)
    assert len(cs) == 3 and 0 < cs[0] < cs[1] < cs[2] < end
    pieces, off = [], 1
    for skip, cap in block_windows(cs, end):
        pieces.append([0, bits, off, cap, skip])
        off += cap
    out = np.full(off + 64, 0xAB, np.uint8)
    rc, ln, status, rounds, _ = run_decode(remu, c, data, pieces, out, W, S, K)
    assert rc == 0 and not any(status), status
    want = np.full(out.size, 0xAB, np.uint8)
    for (_, _, o, cap, skip), n, r in zip(pieces, ln, rounds):
        assert n == cap and r == rounds_for(cs, skip, cap), (skip, cap, n, r, cs)
        want[o: o + cap] = ref[skip: skip + cap]
    assert np.array_equal(out, want)
    out = np.full(64, 0xAB, np.uint8)
    rc, ln, status, rounds, _ = run_decode(remu, c, data, [[0, bits, 8, 20, end - 5]], out, W, S, K)
    assert rc == 0 and status == [ERR_FORMAT] and ln == [5] and rounds == [4]
    assert np.array_equal(out[8:13], ref[end - 5:]) and (out[:8] == 0xAB).all() and (out[13:] == 0xAB).all()


def _round_model(c, data, bits, S, G, W):
    """The rounds of one stream in Python, walking the tree bit by bit (no
    table, no K): region j > 0 of a round is entered in the node a chain from
    the root reaches over the G bits before it, region 0 in the carried one;
    a lane whose predecessor left in another node than it was entered in
    takes that node and walks again, until none does.  (rounds, fix rounds
    that changed a lane, the most of them in one round, regions walked
    again): hh_batch_emu_decode's stats[3..6]."""
    iz, io = np.asarray(c.izero).tolist(), np.asarray(c.ione).tolist()
    bit = np.unpackbits(np.asarray(data, np.uint8), bitorder="little").tolist()
    memo = {}

    def walk(v, at, n):
        if (v, at, n) not in memo:
            u = v
            for b in bit[at: at + n]:
                u = io[u] if b else iz[u]
                if iz[u] < 0:
                    u = 0
            memo[(v, at, n)] = u
        return memo[(v, at, n)]

    NL = 64 * W
    rounds = fixes = most = again = carry = 0
    for R0 in range(0, bits, NL * S):
        rounds += 1
        at = [R0 + j * S for j in range(NL)]
        nb = [max(0, min(S, bits - a)) for a in at]
        ent = [carry] + [walk(0, at[j] - G, G) if G and nb[j] else 0 for j in range(1, NL)]
        x = [walk(ent[j], at[j], nb[j]) for j in range(NL)]
        fr = 0
        while True:
            px, any_ = list(x), False
            for j in range(1, NL):
                if nb[j] and px[j - 1] != ent[j]:
                    ent[j], any_ = px[j - 1], True
                    again += 1
                    x[j] = walk(ent[j], at[j], nb[j])
            if not any_:
                break
            fr += 1
        fixes += fr
        most = max(most, fr)
        carry = x[NL - 1]
    return rounds, fixes, most, again


@pytest.mark.parametrize("name", [n for n in E.CODE_NAMES + E.SHAPE_NAMES if GEO[n][4]])
def test_guesses_are_the_heads_chains(bemu, name):
    """Every code with a head, at the library's S and K and two waves: a
    stream of three rounds and S + 1 bits.  A wrong guess costs fix rounds and
    no byte (the tests above cannot see one), so the emulator's counts of
    rounds, of fix rounds and of regions walked again are compared with
    _round_model's, which takes every guess from a bit-by-bit chain over the
    G bits before the region: hb_guess's K-bit steps cover exactly those."""
    c = E.any_code(name)
    S, K, _, _, G = GEO[name][:5]
    W = 2
    data, total, _ = E.stream(name, S, 49)
    bits = 3 * W * 64 * S + S + 1
    assert bits <= total
    ref = EC.oracle_prefix(c, data, bits)
    out = np.full(len(ref) + 64, 0xAB, np.uint8)
    rc, out_len, status, st = run_bemu(bemu, c.izero, c.ione, c.sym, data, [[0, bits, 0, len(ref)]], out, W, S=S, K=K)
    assert rc == 0 and out_len[0] == len(ref) and np.array_equal(out[: len(ref)], ref)
    assert (st[0], st[1], st[2]) == (S, G, K), st
    want = _round_model(c, data, bits, S, G, W)
    assert tuple(st[3:7]) == want, (st, want)
    assert want[0] == 4
