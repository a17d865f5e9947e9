"""The record take (hh_decode_batch_take) on the host: the emulator
(tests/emu/hh_take_emu.cpp) compiles the rules the kernels run
(csrc/hh_batch_take_algo.h, csrc/hh_batch_algo.h) and runs the plan record by
record and k_take's packed rounds lane by lane, with a forced share and any W,
so that a few hundred records make a geometry of several workgroups.

The truth needs no model of the decoder: the expected output is the
concatenation of text[offs[r]:offs[r + 1]] for the taken ids, out_offs its
prefix sums, the statuses a dozen-line model() of the contract.  Every output
is filled with 0xAB and compared whole, guard included.
tests/test_gpu_take.py runs the same shapes through Decoder.take_records."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import edge_cases as EC
import shape_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libhh_emu.so")
M64 = (1 << 64) - 1
PAD = 64                    # HH_PAYLOAD_PAD
GUARD = 256
OK, ERR_ARG, ERR_FORMAT, ERR_CAPACITY = 0, -1, -3, -5
GEO = {**E.CODE_GEOMETRY, **E.SHAPE_GEOMETRY}
ALL_NAMES = E.CODE_NAMES + E.SHAPE_NAMES
# k_take's waves per workgroup (hbt_pick_waves): k_batch's W where the LDS allows
TAKE_W = {"kjv": 6, "byte256": 6, "fixed2": 16, "fixed1": 16, "caterpillar40": 7, "complete5": 16, "complete7": 16,
          "complete8": 14, "lattice3": 16, "lattice5": 16, "lattice6": 16, "split7": 16, "random128": 11,
          "random200": 7, "random12": 13, "caterpillar64": 7}


@pytest.fixture(scope="module")
def temu():
    if not os.path.exists(EMU):
        pytest.skip("tests/emu/libhh_emu.so not built (make emu)")
    L = C.CDLL(EMU)
    L.hh_take_emu.restype = C.c_int64
    L.hh_take_emu.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hh_take_row_ok.restype = C.c_int32
    L.hh_take_row_ok.argtypes = [C.c_uint64] * 5
    L.hh_take_fate.restype = C.c_int32
    L.hh_take_fate.argtypes = [C.c_int32] + [C.c_uint64] * 4
    L.hh_take_sat_add.restype = C.c_uint64
    L.hh_take_sat_add.argtypes = [C.c_uint64] * 2
    L.hh_take_share.restype = C.c_uint64
    L.hh_take_share.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    L.hh_take_pick_waves.restype = C.c_uint32
    L.hh_take_pick_waves.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)]
    return L


# ---------------------------------------------------------------------------
# The contract in Python integers
# ---------------------------------------------------------------------------
def row_ok(r, nrec, data_off, bits, data_bytes):
    if r >= nrec or data_off % 4:
        return False
    return bits == 0 or data_off + (bits + 7) // 8 + PAD <= data_bytes


def model(index, ids, data_bytes, out_bytes, counts=None):
    """(out_offs, status, delivered) of a take: index rows of (data_off, bits,
    out_off, cap) in Python integers, ids a list or None, counts[r] the
    symbols row r's stream really holds (default: its cap)."""
    nrec = len(index)
    ids = list(range(nrec)) if ids is None else ids
    offs, status, deliv, off = [], [], [], 0
    for r in ids:
        ok = r < nrec and row_ok(r, nrec, index[r][0], index[r][1], data_bytes)
        ln = index[r][3] if ok else 0
        offs.append(off)
        off = min(off + ln, M64)
        c = (index[r][3] if counts is None else counts[r]) if ok else 0
        if not ok:
            status.append(ERR_ARG)
        elif off > out_bytes:
            status.append(ERR_CAPACITY)
        else:
            status.append(OK if c == ln else ERR_FORMAT)
        deliv.append(min(c, ln) if status[-1] in (OK, ERR_FORMAT) else 0)
    return offs + [off], status, deliv


def summary_of(offs, status):
    bad = [j for j, s in enumerate(status) if s != OK]
    return {"total_len": sum(offs[j + 1] - offs[j] for j, s in enumerate(status) if s == OK), "n_failed": len(bad),
            "first_failed": bad[0] if bad else 0xffffffff, "first_status": status[bad[0]] if bad else OK}


def expected(size, offs, deliv, ids, recs):
    """The output buffer: 0xAB but for the delivered prefix of every taken
    record; recs[r] the symbols row r's stream decodes to."""
    want = np.full(size, 0xAB, np.uint8)
    for j, r in enumerate(ids):
        if deliv[j]:
            want[offs[j]: offs[j] + deliv[j]] = recs[r][: deliv[j]]
    return want


# ---------------------------------------------------------------------------
# Records with chosen bits
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _alphabet(name):
    c = E.any_code(name)
    L = EC._lengths(c.izero, c.ione, c.sym)
    syms = np.array(sorted(L), np.uint8)
    lens = np.array([L[int(s)] for s in syms], np.int64)
    p = np.array([2.0 ** -int(l) for l in lens])
    by_len = {}
    for s, l in zip(syms.tolist(), lens.tolist()):
        by_len.setdefault(l, s)
    lut = np.zeros(256, np.int64)
    lut[syms] = lens
    return syms, lens, p / p.sum(), by_len, lut


def record(rng, name, target):
    """Symbols whose codes take `target` bits, or the most below it that the
    code's lengths can add up to (at least one symbol): random ones, then a
    tail chosen by a coin-change table over the code's lengths."""
    syms, lens, p, by_len, lut = _alphabet(name)
    maxlen, minlen = int(lens.max()), int(lens.min())
    if target <= 0:
        return np.zeros(0, np.uint8)
    head = np.zeros(0, np.uint8)
    room = maxlen * minlen + 4 * maxlen              # (past the lengths' Frobenius number)
    if target > room:
        draw = rng.choice(syms, size=(target - room) // minlen + 1, p=p)
        k = int(np.searchsorted(np.cumsum(lut[draw]), target - room, side="right"))
        head = draw[:k].astype(np.uint8)
    rem = target - int(lut[head].sum())
    via = [None] * (rem + 1)
    via[0] = 0
    for v in range(1, rem + 1):
        for l in by_len:
            if l <= v and via[v - l] is not None:
                via[v] = l
                break
    while via[rem] is None:
        rem -= 1
    tail = []
    while rem:
        tail.append(by_len[via[rem]])
        rem -= via[rem]
    if not len(head) and not tail:
        tail = [by_len[minlen]]
    return np.concatenate([head, np.array(tail, np.uint8)])


@functools.lru_cache(maxsize=None)
def layout(name, W, S):
    """The records of the round-edge shapes for rounds of NL = 64 W slots of S
    bits, as (text, offs, data, index, marks): an encode_ragged of
      1500 empties;
      records of k S, k S + 1, k S - 1 bits for k = 1, 2, 3, and of 1 bit;
      one-region records up to a two-region record that ENDS in round 0's last
      slot; round 1 from its slot 0 with one-region records up to a
      three-region record that STARTS in its last slot (the carry); 1500
      empties; one-region records to the end of round 2;
      a LONG stream of 2.5 rounds between one-region records, whose last round
      it shares with them;
      1500 empties.
    The lengths are nudged by record() to what the code's lengths can reach;
    marks names the special records and the slots they were laid at, which the
    test checks against the encoder's bits."""
    NL = 64 * W
    rng = np.random.default_rng([NL, S, E.name_index(name)])
    recs, slot, marks = [], 0, {}

    def put(target):
        nonlocal slot
        r = record(rng, name, target)
        recs.append(r)
        slot += -(-int(_alphabet(name)[4][r].sum()) // S)
        return len(recs) - 1

    def empties(n):
        recs.extend([np.zeros(0, np.uint8)] * n)

    def fill_to(end):
        while slot < end:
            put(int(rng.integers(1, S + 1)))
        assert slot == end

    empties(1500)
    for k in (1, 2, 3):
        for d in (0, 1, -1):
            put(k * S + d)
    put(1)
    fill_to(NL - 2)
    marks["ends_last"] = put(2 * S - 5)
    assert slot == NL
    marks["starts_first"] = put(S // 2)
    fill_to(2 * NL - 1)
    marks["carry"] = put(3 * S - 7)
    empties(1500)
    marks["inside_empties"] = len(recs) - 1
    fill_to(3 * NL)
    put(S - 1)
    marks["long"] = put(2 * NL * S + NL * S // 2)
    marks["long_slot"] = slot
    fill_to(-(-slot // NL) * NL + 3)
    empties(1500)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    text = np.concatenate(recs).astype(np.uint8)
    data, index = E.any_code(name).tree().encode_ragged(text, offs)
    return text, offs, data, index, marks


def records_of(text, offs):
    return [text[int(a): int(b)] for a, b in zip(offs[:-1], offs[1:])]


def run_emu(L, name, data, index, ids, out_bytes, W, S, K, share=0, grid=1, shift=0, data_bytes=None):
    """One emulated take into a 0xAB buffer of out_bytes + GUARD bytes, shift
    bytes into an aligned array: (rc, out, out_offs, status, summary, stats)."""
    c = E.any_code(name)
    iz = np.ascontiguousarray(c.izero, np.int32)
    io = np.ascontiguousarray(c.ione, np.int32)
    sy = np.ascontiguousarray(c.sym, np.uint8)
    data = np.ascontiguousarray(data, np.uint8)
    index = np.ascontiguousarray(index, np.uint64).reshape(-1, 4)
    nrec = index.shape[0]
    idv = None if ids is None else np.ascontiguousarray(ids, np.uint64)
    m = nrec if ids is None else idv.size
    buf = np.full(shift + out_bytes + GUARD, 0xAB, np.uint8)
    out = buf[shift:]
    offs = np.full(m + 1, 77, np.uint64)
    status = np.full(m, 77, np.int32)
    summ = np.full(4, 77, np.int64)
    st = np.zeros(13, np.int64)
    rc = L.hh_take_emu(iz.ctypes.data, io.ctypes.data, sy.ctypes.data, len(iz), data.ctypes.data,
                       data.size if data_bytes is None else data_bytes, index.ctypes.data, nrec,
                       None if idv is None else idv.ctypes.data, m, S, K, W, share, grid, out.ctypes.data, out_bytes,
                       offs.ctypes.data, status.ctypes.data, summ.ctypes.data, st.ctypes.data)
    summary = {"total_len": int(summ[0]), "n_failed": int(summ[1]), "first_failed": int(summ[2]),
               "first_status": int(summ[3])}
    return int(rc), out, offs.tolist(), status.tolist(), summary, st.tolist()


def check_take(got, index, ids, data_bytes, out_bytes, recs, counts=None):
    """A take's results against the model and the text, the whole buffer."""
    rc, out, offs, status, summary, _ = got
    idx = np.asarray(index, np.uint64).tolist()
    ids_l = list(range(len(idx))) if ids is None else [int(i) for i in ids]
    w_offs, w_status, deliv = model(idx, ids_l, data_bytes, out_bytes, counts)
    assert rc == 0
    assert offs == w_offs
    assert status == w_status, [(j, a, b) for j, (a, b) in enumerate(zip(status, w_status)) if a != b][:8]
    want = expected(out.size, w_offs, deliv, ids_l, recs)
    assert np.array_equal(out, want), int(np.argmax(out != want))
    assert summary == summary_of(w_offs, w_status)


# ---------------------------------------------------------------------------
# The rules
# ---------------------------------------------------------------------------
def test_row_rules_and_sums(temu):
    """hbt_row_ok in its corners (never sent to a GPU as addresses): an id at
    and past nrec, data_off off a word, a payload that ends at, one byte past
    and far past data_bytes, data_off and bits near 2^64; the saturating sum;
    the fates; a share is whole rounds and never 0."""
    for r, nrec, d, b, db in [(0, 1, 0, 8, 65), (0, 1, 0, 8, 64), (1, 1, 0, 8, 999), (M64, 5, 0, 8, 999),
                              (0, 1, 2, 8, 999), (0, 1, 1, 0, 999), (0, 1, 4, 0, 0), (0, 1, M64 - 3, 8, M64),
                              (0, 1, M64 - 3, 0, 10), (0, 1, 0, M64, M64), (0, 1, 8, 8 * (M64 // 8), M64),
                              (0, 1, 1 << 63, 1 << 63, M64), (0, 1, 900, 8, 964), (0, 1, 900, 9, 965)]:
        assert bool(temu.hh_take_row_ok(r, nrec, d, b, db)) == row_ok(r, nrec, d, b, db), (r, nrec, d, b, db)
    for a, b in [(0, 0), (1, M64 - 1), (1, M64), (M64, M64), (1 << 63, 1 << 63), (5, 7)]:
        assert temu.hh_take_sat_add(a, b) == min(a + b, M64)
    STREAM = 0x7ffffffe
    assert temu.hh_take_fate(0, 8, 1, 1, 10) == ERR_ARG
    assert temu.hh_take_fate(1, 8, 1, 11, 10) == ERR_CAPACITY and temu.hh_take_fate(1, 0, 0, 11, 10) == ERR_CAPACITY
    assert temu.hh_take_fate(1, 8, 1, M64, M64) == STREAM and temu.hh_take_fate(1, 8, 1, 10, 10) == STREAM
    assert temu.hh_take_fate(1, 0, 0, 10, 10) == OK
    assert temu.hh_take_fate(1, 0, 3, 10, 10) == ERR_FORMAT and temu.hh_take_fate(1, 8, 0, 10, 10) == ERR_FORMAT
    for nslots, grid, NL in [(0, 4, 128), (1, 4, 128), (128, 1, 128), (129, 1, 128), (10000, 7, 384), (1 << 60, 3, 1024)]:
        s = temu.hh_take_share(nslots, grid, NL, 0)
        assert s and s % NL == 0 and s * grid >= nslots and (s - NL) * grid < max(nslots, 1), (nslots, grid, NL, s)
    assert temu.hh_take_share(1000, 9, 128, 130) == 256


def test_waves_fit_the_lds(temu):
    """k_take's W for every table size and region: at most k_batch's (the
    marks and the streams' rows by ordinal take 24 bytes of LDS per slot that
    k_batch does not need), the values of DESIGN.md section 15."""
    for name in ALL_NAMES:
        S, K, r, _, _, Wb, ns = GEO[name]
        minlen = E.any_code(name).tree().info()["minlen"]
        lg = max(K, 5)                      # (HH_FSM_ET_LG)
        tabb = (((ns << lg) * 8 + ((ns << r) * 8 if r else 0) + ns * 8 + ns) + 15) & ~15
        wb = C.c_uint32(0)
        wt = temu.hh_take_pick_waves(tabb, S, minlen, 160 * 1024, C.byref(wb))
        assert wb.value == Wb, (name, wb.value, Wb)
        assert 1 <= wt <= Wb and wt == TAKE_W[name], (name, wt, Wb)


# ---------------------------------------------------------------------------
# Packed rounds
# ---------------------------------------------------------------------------
def _case(name, W):
    S, K = GEO[name][:2]
    text, offs, data, index, marks = layout(name, W, S)
    return S, K, text, offs, data, index, marks, records_of(text, offs)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_round_edges(temu, name):
    """layout()'s records at W = 2, all taken in order, by one workgroup and
    by shares of one round (the long stream straddles two share edges: the
    workgroup that starts it finishes it, the next begins at the next stream):
    bytes, offsets, statuses, summary.  The special records lie where layout()
    says: checked from the encoder's bits."""
    W = 2
    S, K, text, offs, data, index, marks, recs = _case(name, W)
    NL = 64 * W
    reg = -(-index[:, 1].astype(np.int64) // S)
    slot0 = np.cumsum(reg) - reg
    e = marks["ends_last"]
    assert slot0[e] + reg[e] == NL and reg[e] == 2
    assert slot0[marks["starts_first"]] == NL
    k = marks["carry"]
    assert slot0[k] == 2 * NL - 1 and reg[k] >= 2
    g = marks["long"]
    assert reg[g] >= 2 * NL + NL // 2 - 1 and slot0[g] % NL == 1
    bits = set(index[:, 1].tolist())
    if name not in ("fixed1", "fixed2") and not name.startswith(("complete", "lattice")):
        assert {S, S + 1, S - 1, 2 * S, 2 * S + 1, 2 * S - 1, 3 * S, 3 * S + 1, 3 * S - 1} <= bits, name
    total = int(offs[-1])
    for share, grid in ((0, 1), (NL, 0), (0, 5)):
        got = run_emu(temu, name, data, index, None, total, W, S, K, share=share, grid=grid)
        check_take(got, index, None, data.size, total, recs)
        st = got[5]
        assert st[7] == int((reg > 0).sum()) and st[8] == int(reg.sum()) and st[11] == 0
        assert st[3] >= -(-st[8] // NL)
        if share:
            assert st[9] >= 4 and st[12] >= NL - 32


@pytest.mark.parametrize("W", [1, 16])
def test_round_edges_other_waves(temu, W):
    S, K, text, offs, data, index, marks, recs = _case("kjv", W)
    total = int(offs[-1])
    for share in (0, 64 * W):
        got = run_emu(temu, "kjv", data, index, None, total, W, S, K, share=share)
        check_take(got, index, None, data.size, total, recs)


@pytest.mark.parametrize("name", ["kjv", "byte256", "fixed1", "lattice5", "caterpillar64"])
def test_ids(temu, name):
    """None is covered above; a random permutation, a subset, every id twice,
    one record 1000 times, and ids equal to nrec and 2^64 - 1 among good
    ones: HH_ERR_ARG, length 0, the neighbours exact."""
    W = 2
    S, K, text, offs, data, index, marks, recs = _case(name, W)
    nrec = index.shape[0]
    rng = np.random.default_rng(5)
    perm = rng.permutation(nrec).astype(np.uint64)
    subset = np.sort(rng.choice(nrec, nrec // 3, replace=False)).astype(np.uint64)
    twice = np.repeat(np.arange(nrec, dtype=np.uint64), 2)
    one = np.full(1000, marks["carry"], np.uint64)
    bad = np.arange(1490, 1600, dtype=np.uint64)
    bad[[3, 50, 51, 109]] = [nrec, M64, nrec + 1, M64 - 1]
    for ids in (perm, subset, twice, one, bad):
        total = int(sum(index[int(i), 3] for i in ids if i < nrec))
        got = run_emu(temu, name, data, index, ids, total, W, S, K, share=128)
        check_take(got, index, ids, data.size, total, recs)


def test_empties_and_nothing(temu):
    """All records empty: every status 0, nothing written, no stream, no
    round.  m == 0: the empty summary, nothing else written.  ids == NULL
    with m != nrec is the host's HH_ERR_ARG (the emulator takes m from nrec
    then; the C call is checked on the GPU)."""
    index = np.zeros((3000, 4), np.uint64)
    got = run_emu(temu, "kjv", np.zeros(128, np.uint8), index, None, 16, 2, 256, 7)
    check_take(got, index, None, 128, 16, [np.zeros(0, np.uint8)] * 3000)
    assert got[5][3] == 0 and got[5][7] == 0
    rc, out, offs, status, summary, st = run_emu(temu, "kjv", np.zeros(128, np.uint8), index,
                                                 np.zeros(0, np.uint64), 16, 2, 256, 7)
    assert rc == 0 and (out == 0xAB).all() and offs == [77]
    assert summary == {"total_len": 0, "n_failed": 0, "first_failed": 0xffffffff, "first_status": 0}


def test_bad_rows(temu):
    """data_off odd, a payload past data_bytes, data_off near 2^64:
    HH_ERR_ARG, length 0, nothing read or written for them; the others
    exact."""
    W = 2
    S, K, text, offs, data, index, marks, recs = _case("kjv", W)
    idx = index.copy()
    a, b, c = 1510, 1511, marks["carry"]
    idx[a, 0] += 2
    idx[b, 0] = data.size - PAD
    idx[c, 0] = M64 - 3
    total = int(idx[:, 3].sum()) - int(idx[[a, b, c], 3].sum())
    got = run_emu(temu, "kjv", data, idx, None, total, W, S, K, share=128)
    check_take(got, idx, None, data.size, total, recs)
    assert got[3][a] == got[3][b] == got[3][c] == ERR_ARG


def disagreements(name, index, marks, recs, S, NL):
    """(what, row, field, value) of the index edits: a short record that
    shares its round with good ones, and the long stream.  The lowered bits
    end the stream one bit into its last symbol but one: one symbol fewer,
    whatever the tail rule adds."""
    lut = _alphabet(name)[4]
    short, lg = marks["starts_first"] + 1, marks["long"]
    while index[short, 1] < 16 or index[short, 3] < 2:
        short += 1
    out = []
    for who, r in (("short", short), ("long", lg)):
        cap, bits = int(index[r, 3]), int(index[r, 1])
        out += [(who + "+1", r, 3, cap + 1), (who + "+round", r, 3, cap + NL * S), (who + "-1", r, 3, cap - 1),
                (who + "=0", r, 3, 0), (who + " bits", r, 1, int(lut[recs[r][:-2]].sum()) + 1),
                (who + " bits=0", r, 1, 0)]
    return out


def true_count(name, data, row):
    """The symbols a row's stream holds and what it decodes to (the oracle's
    chain decode of its bits: for a stream cut short, with the tail rule)."""
    d, b = int(row[0]), int(row[1])
    if b == 0:
        return np.zeros(0, np.uint8)
    return EC.oracle_prefix(E.any_code(name), data[d:], b)


@pytest.mark.parametrize("name", ["kjv", "byte256", "complete7", "caterpillar40"])
def test_index_and_data_disagree(temu, name):
    """One row's cap raised by 1 and by a whole round, lowered by 1 and to 0,
    its bits lowered so that the stream ends early, and bits 0 under a
    length: HH_ERR_FORMAT on that record alone, exactly min(c, len) bytes
    delivered, the rest of its range still 0xAB, every other record exact --
    for a record that shares its round with good ones and for the long
    stream (both copy-out paths: the emulator says which ran)."""
    W = 2
    S, K, text, offs, data, index, marks, recs = _case(name, W)
    for what, r, field, value in disagreements(name, index, marks, recs, S, 64 * W):
        idx = index.copy()
        idx[r, field] = value
        dec = true_count(name, data, idx[r])
        counts = idx[:, 3].tolist()
        counts[r] = len(dec)
        rr = list(recs)
        rr[r] = dec
        total = int(idx[:, 3].sum())
        got = run_emu(temu, name, data, idx, None, total, W, S, K, share=256)
        check_take(got, idx, None, data.size, total, rr, counts)
        assert got[3][r] == ERR_FORMAT and got[4]["n_failed"] == 1, what
        assert got[5][11] >= (1 if idx[r, 1] and idx[r, 3] else 0), (what, got[5])


@pytest.mark.parametrize("name", ["kjv", "fixed2"])
def test_capacity(temu, name):
    """out_bytes equal to the total, one byte less, cutting a record in half,
    0: the records past it get HH_ERR_CAPACITY, out_offs is complete, nothing
    is written at or beyond out_bytes."""
    W = 2
    S, K, text, offs, data, index, marks, recs = _case(name, W)
    total = int(offs[-1])
    k = marks["carry"]
    for ob in (total, total - 1, int(offs[k]) + int(index[k, 3]) // 2, 0):
        got = run_emu(temu, name, data, index, None, ob, W, S, K, share=128)
        check_take(got, index, None, data.size, ob, recs)
        assert got[2][-1] == total


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_alignment(temu, shift):
    W = 2
    S, K, text, offs, data, index, marks, recs = _case("kjv", W)
    total = int(offs[-1])
    got = run_emu(temu, "kjv", data, index, None, total, W, S, K, share=128, shift=shift)
    check_take(got, index, None, data.size, total, recs)


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_scan_tiles(temu, m):
    W = 2
    S, K, text, offs, data, index, marks, recs = _case("kjv", W)
    ids = np.arange(1400, 1400 + m, dtype=np.uint64)
    total = int(index[1400: 1400 + m, 3].sum())
    got = run_emu(temu, "kjv", data, index, ids, total, W, S, K)
    check_take(got, index, ids, data.size, total, recs)


def test_blocked_index(temu):
    """A list from the blocked encoder has the same fields: a blocked buffer
    taken by block id."""
    text, B, data, index = E.blocked("kjv", 2, 256)
    recs = [text[i: i + B] for i in range(0, len(text), B)]
    ids = np.array([4, 0, 2, 2, 1, 3], np.uint64)
    total = int(sum(len(recs[int(i)]) for i in ids))
    got = run_emu(temu, "kjv", data, index, ids, total, 2, 256, 7, share=128)
    check_take(got, index, ids, data.size, total, recs)


# ---------------------------------------------------------------------------
# Guesses
# ---------------------------------------------------------------------------
def packed_model(c, data, streams, S, G, W, share):
    """The packed rounds in Python, walking the tree bit by bit (no table, no
    K): the streams (data_off, bits) in take order, a slot per region, shares
    of `share` slots; a lane at its stream's region 0 enters at the root, lane
    0 in the carried node, every other in the node a chain from the root
    reaches over the G bits before its region -- bits of its own stream; a
    lane whose predecessor left in another node than it was entered in takes
    that node and walks again (the exact lanes never), until none does.
    (rounds, fix rounds that changed a lane, the most of them in one round,
    regions walked again): hh_take_emu's stats[3..6]."""
    iz, io = np.asarray(c.izero).tolist(), np.asarray(c.ione).tolist()
    bit = np.unpackbits(np.asarray(data, np.uint8), bitorder="little").tolist()

    def walk(v, at, n):
        for b in bit[at: at + n]:
            v = io[v] if b else iz[v]
            if iz[v] < 0:
                v = 0
        return v

    NL = 64 * W
    slots, first = [], []
    for k, (d, b) in enumerate(streams):
        first.append(len(slots))
        slots += [(k, q) for q in range(-(-b // S))]
    rounds = fixes = most = again = 0
    wgs = {}
    for k, f in enumerate(first):
        wgs.setdefault(f // share, []).append(k)
    for ks in wgs.values():
        mine = slots[first[ks[0]]: first[ks[-1]] + -(-streams[ks[-1]][1] // S)]
        carry = 0
        for lo in range(0, len(mine), NL):
            rounds += 1
            lanes = mine[lo: lo + NL]
            at = [8 * streams[k][0] + q * S for k, q in lanes]
            nb = [max(0, min(S, streams[k][1] - q * S)) for k, q in lanes]
            exact = [j == 0 or q == 0 for j, (k, q) in enumerate(lanes)]
            ent = [(0 if q == 0 else carry) if exact[j] else (walk(0, at[j] - G, G) if G else 0)
                   for j, (k, q) in enumerate(lanes)]
            x = [walk(ent[j], at[j], nb[j]) for j in range(len(lanes))]
            fr = 0
            while True:
                px, any_ = list(x), False
                for j in range(1, len(lanes)):
                    if not exact[j] and px[j - 1] != ent[j]:
                        ent[j], any_ = px[j - 1], True
                        again += 1
                        x[j] = walk(ent[j], at[j], nb[j])
                if not any_:
                    break
                fr += 1
            fixes += fr
            most = max(most, fr)
            carry = x[-1]
    return rounds, fixes, most, again


@pytest.mark.parametrize("name", [n for n in ALL_NAMES if GEO[n][4]] + ["complete7"])
def test_guesses_are_the_own_streams_heads(temu, name):
    """No byte-exact test sees a wrong guess: it costs fix rounds and no byte.
    So the emulator's counts of rounds, fix rounds and regions walked again
    are pinned against packed_model's, whose guesses are bit-by-bit chains
    over the G bits before a region.  Were the lanes at a stream's region 0
    to guess instead of starting at the root, or a lane to take its guess
    from a row of another stream, the counts would differ: the records here
    mostly end inside a code's worth of padding bits, so the row before a
    stream's first region does not lead to the root."""
    W = 1
    S, K, G = GEO[name][0], GEO[name][1], GEO[name][4]
    c = E.any_code(name)
    rng = np.random.default_rng([9, E.name_index(name)])
    targets = [int(rng.integers(1, 4 * S)) for _ in range(150)] + [3 * 64 * S + 40] + \
              [int(rng.integers(1, 2 * S)) for _ in range(40)]
    recs = [record(rng, name, t) for t in targets]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    text = np.concatenate(recs)
    data, index = c.tree().encode_ragged(text, offs)
    total = int(offs[-1])
    share = 2 * 64 * W
    got = run_emu(temu, name, data, index, None, total, W, S, K, share=share)
    check_take(got, index, None, data.size, total, recs)
    st = got[5]
    assert (st[0], st[1], st[2]) == (S, G, K), st
    want = packed_model(c, data, [(int(d), int(b)) for d, b in index[:, :2].tolist()], S, G, W, share)
    assert tuple(st[3:7]) == want, (st, want)
    assert want[0] >= 6
