"""k_batch (csrc/hh_batch.hip) and the kernels around it over the geometry a
tree gives them.  hh_decoder_set_tree derives the region bits S, the emission
step K, the remainder step r = S mod K with its `er` table, the count step
bits cb, the batch's head G and the waves per round W from the tree alone;
tests/test_gpu_batch.py, test_gpu_batch_items.py and test_gpu_blocks_read.py
are careful about lengths, alignments, capacities and stream order but run
five codes.  shape_cases' family fills the rest of the table: the first GPU
runs of k_batch with r in {3, 6}, of K = 6 with a remainder step, of 160- and
192-bit regions, of 12 and 14 waves and of a head of 105 bits
(test_geometry_cells holds the library to that).  tests/test_emu_shapes.py
runs the same shapes through the emulator.

Two device-only pieces of the planners run here for the first time as well:
k_read_scan's over-budget branch across its 1024-read tiles
(test_reads_past_the_budget) and the summaries' last-workgroup code with
failures in several 256-thread workgroups (test_summaries_across_workgroups).

As in the files above every output is 0xAB first and compared whole, byte
for byte."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_cases as EC
import shape_cases as E
from test_blocks_read import block_windows, budget, model, round_counts, rounds_for
from test_emu_batch import batch_cuts
from test_gpu_batch import GUARD, _check_exact, _clean, _complete_tree, _packed
from test_gpu_batch_items import _dev_items
from test_gpu_blocks_read import _bible, _dev, _pack, _same, _want

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FORMAT, ERR_CAPACITY = -1, -3, -5
NONE = 0xffffffff
LDS = 160 * 1024
GEO = {**E.CODE_GEOMETRY, **E.SHAPE_GEOMETRY}
_REFS = {}                 # (code, data_off, bits) -> the oracle's decode


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module")
def enc(hh):
    e = hh.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _drop_buffers():
    yield
    import torch
    _REFS.clear()
    E.blocked.cache_clear()
    _bible.cache_clear()
    torch.cuda.empty_cache()


def _refs(name, data, keys):
    """test_gpu_batch.py's _refs for a shape as well: the oracle's decodes of
    `bits` bits from byte data_off of data, for (data_off, bits) in keys, each
    computed once per stream (data: one array per name in a test)."""
    c = E.any_code(name)
    miss = [k for k in dict.fromkeys(keys) if (name,) + k not in _REFS]
    if miss:
        with ThreadPoolExecutor(8) as ex:
            for k, r in zip(miss, ex.map(lambda k: EC.oracle_prefix(c, data[k[0]:], k[1]), miss)):
                _REFS[(name,) + k] = r
    return [_REFS[(name,) + k] for k in keys]


def _decoder(hh, name):
    c = E.any_code(name)
    dec = hh.Decoder(0, flags=c.flags)
    dec.set_tree(c.tree())
    return dec


def test_geometry_cells(hh, capsys):
    """What set_tree chose for every shape and every code of CODE_NAMES
    (Decoder.geometry(): host fields, no kernel is launched): it agrees with
    tile_bits() and batch_round_tiles(), fits the LDS, r = S mod K, the head
    is whole K-bit steps; it is the table shape_cases records (which the
    emulator tests take their S and K from); and the table as a whole has the
    cells this file is there for: r in {0, 2, 3, 4, 6}, K in {4, 5, 6, 7}, S
    in {160, 192, 224, 256}, both count steps, 16 waves and three other wave
    counts, and a code that is not fixed-length on a lattice coarser than one
    bit."""
    got, lattice = {}, []
    for name in E.CODE_NAMES + E.SHAPE_NAMES:
        dec = _decoder(hh, name)
        try:
            g = dec.geometry()
            assert g["S"] == dec.tile_bits() // 64 and dec.tile_bits() % 64 == 0 and g["W"] == dec.batch_round_tiles()
            assert 0 < g["lds"] <= LDS and g["r"] == g["S"] % g["K"] and g["G"] % g["K"] == 0 and g["G"] <= g["S"], g
            assert g["cb"] == (8 if g["ns"] <= 127 else 7) and g["ns"] == int((np.asarray(dec._tree.izero) >= 0).sum())
            got[name] = tuple(g[k] for k in E.GEOMETRY_KEYS)
            if not E.any_code(name).complete and dec._tree.info()["len_gcd"] > 1:
                lattice.append(name)
        finally:
            dec.close()
    with capsys.disabled():
        print("\n" + "\n".join(f"geometry {n:14s} " + " ".join(f"{k}={v}" for k, v in zip(E.GEOMETRY_KEYS, t))
                               for n, t in got.items()))
    assert got == GEO, {n: (t, GEO[n]) for n, t in got.items() if t != GEO[n]}     # (shape_cases' tables follow the library)
    col = lambda k: {t[E.GEOMETRY_KEYS.index(k)] for t in got.values()}
    assert col("r") >= {0, 2, 3, 4, 6} and col("K") == {4, 5, 6, 7} and col("S") >= {160, 192, 224, 256}
    assert col("cb") == {7, 8} and 16 in col("W") and len(col("W") - {16}) >= 3, col("W")
    assert lattice, "no non-fixed code with a code-length gcd above 1"
    bare = hh.Decoder(0)
    try:
        with pytest.raises(hh.HipHuffError) as e:
            bare.geometry()
        assert e.value.status == ERR_ARG
        bare.set_tree(hh.Tree(*_complete_tree(11)))              # past the state machine's 255 states
        with pytest.raises(hh.HipHuffError) as e:
            bare.geometry()
        assert e.value.status == -10
    finally:
        bare.close()


@pytest.mark.parametrize("name", E.SHAPE_NAMES)
def test_breakpoints(hh, name):
    """test_gpu_batch.py::test_breakpoints for the shape: one stream of 3 W
    tiles and S + 2 bits, every batch_cuts prefix of it in one batch, the
    outputs back to back from offset 1 with exact capacities -- bytes, out_len
    and statuses the oracle's, nothing written outside, the stats the batched
    decode's.  Then the same batch from a device list: the same buffer."""
    import torch
    dec = _decoder(hh, name)
    try:
        TBITS = dec.tile_bits()
        S = TBITS // 64
        W = dec.batch_round_tiles()
        assert (S, W) == (GEO[name][0], GEO[name][5])
        data, bits, _ = E.stream(name, S, 3 * W)
        cuts = batch_cuts(S, W, dec._tree.info()["maxlen"], bits)
        assert cuts[-1] == 3 * W * TBITS + S + 1 and {W * TBITS, 2 * W * TBITS, 2 * W * TBITS + 1} <= set(cuts)
        keys = [(0, b) for b in cuts]
        refs = _refs(name, data, keys)
        items, end = _packed(keys, refs, 1)
        d_data = torch.from_numpy(data).cuda()
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status = dec.decode_batch(d_data, items, out)
        torch.cuda.synchronize()
        assert not status.any(), status
        _check_exact(out, items, refs, out_len)
        assert _clean(out[:1]) and _clean(out[end:])
        st = dec.stats()
        assert st["state_machine"] == 3 and st["exact_fallback"] == 0 and st["fixed_length"] == 0, st
        assert st["out_len"] == sum(len(r) for r in refs) and st["lanes"] == sum((b + S - 1) // S for b in cuts), st
        out2 = torch.full_like(out, 0xAB)
        out_len2, status2, summ = dec.decode_batch_items(d_data, _dev_items(items), out2, summary=True)
        torch.cuda.synchronize()
        assert not status2.cpu().numpy().any() and np.array_equal(out_len2.cpu().numpy().astype(np.uint64), out_len)
        assert torch.equal(out, out2)
        assert dec.batch_summary(summ) == {"total_len": sum(len(r) for r in refs), "n_failed": 0, "first_failed": NONE,
                                           "first_status": 0}
    finally:
        dec.close()


@pytest.mark.parametrize("name", E.SHAPE_NAMES)
def test_producer_and_windows(hh, enc, name):
    """Five blocks of a little over three rounds of the shape's code, the
    last short.  The device's blocked encode gives the host encoder's bytes
    and items and leaves the items on the device; read_blocks over them, as
    they are: in block 1 the windows of tests/test_blocks_read.py around
    every round boundary, reads across one and two block edges, the whole
    buffer, the empty read at n_syms -- destinations back to back from offset
    1 in shuffled order.  The whole output is the text's slices, every status
    0, the summary the sum."""
    import torch
    dec = _decoder(hh, name)
    try:
        S, W = dec.tile_bits() // 64, dec.batch_round_tiles()
        text, B, data, index = E.blocked(name, W, S)
        n = text.size
        c = E.any_code(name)
        total = data.size - hh.PAYLOAD_PAD
        buf = torch.full((total + hh.PAYLOAD_PAD + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        t = torch.full((index.shape[0], 4), -1, dtype=torch.int64, device="cuda")
        items, got = enc.encode_blocks(dec._tree, torch.from_numpy(text).cuda(), B, buf[:total], items_out=t)
        torch.cuda.synchronize()
        assert got == total and np.array_equal(items, index)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), index)
        assert np.array_equal(buf[:total].cpu().numpy(), data[:total]) and _clean(buf[total:])
        blk = data[int(index[1, 0]):]
        cs = round_counts(c, blk, int(index[1, 1]), 64 * W * S, text[B: 2 * B])
        assert len(cs) == 3 and 0 < cs[0] < cs[2] < B
        assert rounds_for(cs, cs[0] - 1, 1) == 1 and rounds_for(cs, cs[0], 1) == 2
        srcs = [(B + s, l) for s, l in block_windows(cs, B)]
        srcs += [(B - 1, 2), (B - 1, B + 2), (0, n), (n, 0), (n - 1, 1), (4 * B - 1, n - 4 * B + 1)]
        reads, end = _pack(srcs, 1, np.random.default_rng(5))
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        read_len, status, summ = dec.read_blocks(buf[: total + hh.PAYLOAD_PAD], t, n, B, _dev(reads, 3), out, summary=True)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any(), status
        assert np.array_equal(read_len.cpu().numpy().astype(np.uint64), reads[:, 1])
        _same(out, _want(out.numel(), reads, text))
        assert dec.batch_summary(summ) == {"total_len": end - 1, "n_failed": 0, "first_failed": NONE, "first_status": 0}
    finally:
        dec.close()


def _read_call(dec, d_data, d_index, n, B, reads, OB):
    """One read_blocks call into a fresh 0xAB buffer of OB bytes and a guard,
    waited for: (out, read_len, status, summary dict)."""
    import torch
    out = torch.full((OB + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    read_len, status, summ = dec.read_blocks(d_data, d_index, n, B, _dev(reads, 3), out, summary=True, out_bytes=OB)
    torch.cuda.synchronize()
    return out, read_len.cpu().numpy().astype(np.uint64), status.cpu().numpy(), dec.batch_summary(summ)


def _read_summary(reads, stat):
    bad = [i for i, s in enumerate(stat) if s]
    return {"total_len": int(sum(reads[i][1] for i, s in enumerate(stat) if not s)), "n_failed": len(bad),
            "first_failed": bad[0] if bad else NONE, "first_status": stat[bad[0]] if bad else 0}


def test_reads_past_the_budget(hh):
    """k_read_scan's over-budget branch, which only the device runs: 1500
    reads whose pieces pass the budget P = out_bytes / B + 2 m in the scan's
    second tile of 1024 reads.  Only overlapping destinations get there, so
    every read's dst_off is src_off - c for one c and every source lies in a
    span of out_bytes: each output byte has one possible value whatever the
    order of the writes.  698 two-piece reads, then 402 four-piece reads (2 B
    + 2 bytes from k B - 1), the last of which -- read 1099 -- fills the
    budget exactly; of the 400 reads after it those with pieces get
    HH_ERR_ARG and length 0, as do the out-of-range ones, and the empty ones
    stay HH_OK.  Then with 1, 2 and 3 of the two-piece reads made one-piece:
    the budget has that many slots left when the next four-piece read comes,
    which still gets none.  Statuses, lengths and the summary are those of
    test_blocks_read.model(); the output is compared whole."""
    import torch
    B, m, T = 1000, 1500, 400
    text, tree, data, index = _bible(hh, B)
    n = text.size
    k0 = 100
    c, OB = k0 * B - 1, 4 * B + 500
    P = budget(OB, B, m)
    q = OB // B
    assert q % 2 == 0 and P == q + 2 * m
    n4 = q // 2 + T
    n2 = m - T - n4
    rng = np.random.default_rng(1500)
    two = [(k * B - a, a + b) for k, a, b in zip(rng.integers(k0 + 1, k0 + 5, n2).tolist(),
                                                 rng.integers(1, 401, n2).tolist(), rng.integers(1, 401, n2).tolist())]
    four = [(k * B - 1, 2 * B + 2) for k in rng.integers(k0, k0 + 3, n4).tolist()]
    kinds = [(k0 * B - 1, 2 * B + 2), (k0 * B + 7, 0), (n - 10, 20), ((k0 + 2) * B - 3, 9), ((k0 + 1) * B + 5, 10),
             (n, 0), (n + 1, 0)]
    tail = [kinds[k % len(kinds)] for k in range(T)]

    def rows(srcs):
        # (an out-of-range source gets destination 0; an empty read's destination is src_off - c as well)
        return [(s, l, s - c if c <= s <= c + OB - l else 0) for s, l in srcs]

    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_data, d_index = torch.from_numpy(data).cuda(), _dev(index, 4)
        for slack in (0, 1, 2, 3):
            one = [((k0 + 1) * B + 5 + 20 * j, 10) for j in range(slack)]
            reads = rows(one + two[slack:] + four + tail)
            assert len(reads) == m and all(s - c == d for s, l, d in reads if l and s + l <= n)
            stat, first, pieces = model(reads, n, B, OB, P)
            last = n2 + n4 - 1
            assert last > 1024 and not any(stat[: last + 1]) and stat[last + 1] == ERR_ARG
            assert len(pieces) == first[last + 1] == P - slack and first[last] == P - slack - 4
            assert [stat[last + 1 + j] for j in range(7)] == [ERR_ARG, 0, ERR_ARG, ERR_ARG, ERR_ARG, 0, ERR_ARG]
            out, read_len, status, summ = _read_call(dec, d_data, d_index, n, B, np.array(reads, np.uint64), OB)
            assert status.tolist() == stat, (slack, np.flatnonzero(status != np.array(stat))[:8])
            assert read_len.tolist() == [0 if s else l for s, (_, l, _) in zip(stat, reads)]
            failed = [i for i, s in enumerate(stat) if s]
            _same(out, _want(out.numel(), np.array(reads, np.uint64), text, skip=set(failed)))
            assert summ == _read_summary(reads, stat) and summ["first_failed"] == last + 1, summ
    finally:
        dec.close()


def test_summaries_across_workgroups(hh):
    """The summaries' last-workgroup code (the ticket on the done counter,
    the atomic min for first_failed and first_status) with failures in four
    of the six 256-thread workgroups of k_batch_results and k_read_results
    and none in the first; the lowest failing index has another status than
    the later ones.  1500 items: HH_ERR_CAPACITY at 300, HH_ERR_ARG (a
    data_off off a 4-byte boundary) at 600, 601, 900, 1290 and 1499; the
    capacity-failed stream's length counts in total_len.  1500 reads:
    HH_ERR_FORMAT at 300 (a read in the last quarter of a block whose index
    entry says half its bits), HH_ERR_ARG (past n_syms) at the same later
    places; failed reads do not count in total_len.  Each call a second time
    on the same decoder without its lowest failure: the counters are zeroed
    per call, the first failure is then read 600's."""
    import torch
    fails = (600, 601, 900, 1290, 1499)
    assert len({300 // 256} | {i // 256 for i in fails}) == 4 and min(fails) > 300 >= 256
    # items
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        S = dec.tile_bits() // 64
        data, _, _ = E.stream(name, S, 49)
        keys = [(2, 64) if k in fails else (4 * (k // (3 * S)), 1 + k % (3 * S)) for k in range(1500)]
        good = [k for k in keys if k[0] != 2]
        it = iter(_refs(name, data, good))
        refs = [np.zeros(0, np.uint8) if k[0] == 2 else next(it) for k in keys]
        assert len(refs[300]) > 1
        d_data = torch.from_numpy(data).cuda()
        for short in (True, False):
            items, end = _packed(keys, refs, 1, cap=lambda k, ln: 16 if k in fails else ln - 1 if short and k == 300 else ln)
            out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
            out_len, status, summ = dec.decode_batch_items(d_data, _dev_items(items), out, summary=True)
            torch.cuda.synchronize()
            want = [ERR_ARG if k in fails else ERR_CAPACITY if short and k == 300 else 0 for k in range(1500)]
            assert status.cpu().numpy().tolist() == want
            _check_exact(out, items, refs, out_len.cpu().numpy().astype(np.uint64))
            assert dec.batch_summary(summ) == {"total_len": sum(len(r) for r in refs), "n_failed": 5 + short,
                                               "first_failed": 300 if short else 600,
                                               "first_status": ERR_CAPACITY if short else ERR_ARG}
    finally:
        dec.close()
    # reads
    B, bad = 1000, 50
    text, tree, data, index = _bible(hh, B)
    n = text.size
    idx = index.copy()
    idx[bad, 1] //= 2
    half = EC.oracle_prefix(tree, data[int(idx[bad, 0]):], int(idx[bad, 1]))
    assert B // 4 < len(half) < 3 * B // 4 - 50
    rng = np.random.default_rng(1501)
    srcs = []
    while len(srcs) < 1500:
        l = int(rng.integers(0, B))
        s = int(rng.integers(0, n - l + 1))
        if not s // B <= bad <= (s + max(l, 1) - 1) // B:
            srcs.append((s, l))
    for i in fails:
        srcs[i] = (n - 10, 20)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_data = torch.from_numpy(data).cuda()
        for short in (True, False):
            srcs[300] = (bad * B + 3 * B // 4 + 20, 100) if short else (bad * B - 40, 30)
            reads, OB = _pack(srcs, 3)
            stat = [ERR_ARG if i in fails else ERR_FORMAT if short and i == 300 else 0 for i in range(1500)]
            out, read_len, status, summ = _read_call(dec, d_data, _dev(idx, 4), n, B, reads, OB)
            assert status.tolist() == stat
            assert read_len.tolist() == [0 if s else l for s, l in zip(stat, reads[:, 1].tolist())]
            _same(out, _want(out.numel(), reads, text, skip={i for i, s in enumerate(stat) if s}))
            assert summ == _read_summary(reads.tolist(), stat)
            assert (summ["n_failed"], summ["first_failed"], summ["first_status"]) == \
                ((6, 300, ERR_FORMAT) if short else (5, 600, ERR_ARG))
    finally:
        dec.close()
