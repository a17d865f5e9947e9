"""Gathered range reads over a block-coded buffer (hh_decode_blocks_gather,
Decoder.gather_blocks; csrc/hh_batch_gather.hip) on the GPU.  Every case runs
read_blocks and gather_blocks on the same inputs into outputs that are 0xAB
first, and wants the same output bytes, read lengths, statuses and summary
from both, and the text's slices.  tests/test_blocks_gather.py runs the same
rules on the host."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import edge_cases as EC
import shape_cases as E
from test_blocks_read import block_windows, budget, model
from test_gpu_batch import GUARD, _clean, _two_streams
from test_gpu_batch_items import _dev_items, _results
from test_gpu_blocks_read import _bible, _blocked, _dev, _pack, _want

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FORMAT, ERR_UNSUPPORTED = -1, -3, -10
NONE = 0xffffffff
NAMES = EC.CODE_NAMES + E.SHAPE_NAMES


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _drop_buffers():
    yield
    import torch
    E.blocked.cache_clear()
    _blocked.cache_clear()
    _bible.cache_clear()
    _wave1.cache_clear()
    torch.cuda.empty_cache()


def _decoder(hh, name):
    c = E.any_code(name)
    dec = hh.Decoder(0, flags=c.flags)
    dec.set_tree(c.tree())
    return dec


def _five_blocks(name, W, S):
    return _blocked(name, W, S) if name in EC.CODE_NAMES else E.blocked(name, W, S)


def _summary(reads, status):
    bad = np.flatnonzero(status)
    return {"total_len": int(sum(int(reads[i][1]) for i in np.flatnonzero(np.asarray(status) == 0))), "n_failed": int(bad.size),
            "first_failed": int(bad[0]) if bad.size else NONE, "first_status": int(status[bad[0]]) if bad.size else 0}


def _both(dec, d_data, d_index, n, B, reads, size, **kw):
    """read_blocks, then gather_blocks, on the same inputs into two 0xAB
    buffers of size + GUARD bytes: identical output, read_len, status and
    summary.  Returns gather_blocks' (out as numpy, read_len, status, summary)."""
    import torch
    d_reads = reads if torch.is_tensor(reads) else _dev(reads, 3)
    got = []
    for call in (dec.read_blocks, dec.gather_blocks):
        out = torch.full((size + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        read_len, status, summ = call(d_data, d_index, n, B, d_reads, out, summary=True, **kw)
        torch.cuda.synchronize()
        got.append((out.cpu().numpy(), read_len.cpu().numpy().astype(np.uint64), status.cpu().numpy(),
                    dec.batch_summary(summ)))
    (o0, l0, s0, m0), (o1, l1, s1, m1) = got
    bad = np.flatnonzero(o0 != o1)
    assert not bad.size, f"byte {bad[0]}: read_blocks {o0[bad[0]]}, gather_blocks {o1[bad[0]]}; {bad.size} bytes differ"
    assert np.array_equal(l0, l1), np.flatnonzero(l0 != l1)[:10]
    assert np.array_equal(s0, s1), np.flatnonzero(s0 != s1)[:10]
    assert m0 == m1, (m0, m1)
    return got[1]


def _exact(out, want):
    bad = np.flatnonzero(out != want)
    assert not bad.size, f"byte {bad[0]}: got {out[bad[0]]}, want {want[bad[0]]}; {bad.size} bytes differ"


def _round_ends(c, text, rb):
    """The symbols of `text` (one block) complete at each round boundary
    inside its stream: a code that straddles the boundary belongs to the round
    it ends in (test_blocks_read.round_counts, from the code lengths alone)."""
    L = EC._lengths(c.izero, c.ione, c.sym)
    tab = np.zeros(256, np.int64)
    tab[list(L)] = list(L.values())
    cum = np.cumsum(tab[text])
    return [int(np.searchsorted(cum, k * rb, side="right")) for k in range(1, int((cum[-1] - 1) // rb) + 1)]


def _edge_reads(cs, blen):
    """About 40 (skip, len) of a block of blen symbols whose rounds end at cs:
    block_windows' (each round's prefix, a window across and one just past
    every boundary, the rest of the block, the empty ones, the whole block),
    the first and the last byte of every round, small and middling windows
    inside one round."""
    lo, hi = [0] + list(cs), list(cs) + [blen]
    w = block_windows(cs, blen)
    w += [(a, 1) for a in lo] + [(b - 1, 1) for b in hi]
    a, b = lo[-1], hi[-1]
    w += [(a + 5 + 9 * k, 1 + k % 5) for k in range(6)]
    w += [(lo[0] + 40 * k + k, 33 + 3 * k) for k in range(1, 9)]
    return [(s, l) for s, l in w if s + l <= blen]


@pytest.mark.parametrize("name", NAMES)
def test_round_edges(hh, name):
    """Five blocks of a little over three rounds (the last short).  In every
    block the reads of _edge_reads; reads across one, two and three block
    edges, empty reads, a whole block among small ones.  Destinations packed
    back to back from offset 1 in shuffled order, so that neighbours touch at
    every alignment and the staging offset of a 16-byte store differs from
    its destination's in every way."""
    import torch
    dec = _decoder(hh, name)
    try:
        S, W = dec.tile_bits() // 64, dec.batch_round_tiles()
        text, B, data, index = _five_blocks(name, W, S)
        n = text.size
        c = E.any_code(name)
        srcs = []
        for b in range(5):
            blk = text[b * B: (b + 1) * B]
            cs = _round_ends(c, blk, 64 * W * S)
            assert len(cs) == (3 if b < 4 else 1) and 8 < cs[0] < blk.size, (b, cs)
            srcs += [(b * B + s, l) for s, l in _edge_reads(cs, blk.size)]
        srcs += [(B - 1, 2), (B - 1, B + 2), (B - 7, 2 * B + 9), (2 * B - 1, 2 * B + 2), (n, 0), (0, 0), (n - 1, 1),
                 (4 * B - 1, n - 4 * B + 1), (3 * B, B)]
        assert len(srcs) > 150
        for seed in range(20):                                   # the first shuffle that has every alignment
            reads, end = _pack(srcs, 1, np.random.default_rng(seed))
            big = reads[reads[:, 1] > 32]
            if len({int(d) % 16 for d in big[:, 2]}) == 16 == len({int(s - d) % 16 for s, _, d in big.tolist()}):
                break
        assert {int(d) % 16 for d in big[:, 2]} == set(range(16))
        assert len({int(s - d) % 16 for s, _, d in big.tolist()}) == 16
        out, read_len, status, summ = _both(dec, torch.from_numpy(data).cuda(), _dev(index, 4), n, B, reads, end)
        assert not status.any() and np.array_equal(read_len, reads[:, 1])
        _exact(out, _want(out.size, reads, text))
        assert summ == {"total_len": end - 1, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        st = dec.stats()
        assert st.pop("state_machine") == 3 and not any(st.values()), st
    finally:
        dec.close()


@functools.lru_cache(maxsize=None)
def _wave1():
    """A tree whose batch runs one wave per workgroup when its emission step
    is forced to 7 bits: 127 states (the most a 7-bit step takes) and a 2-bit
    code, so that the tables and one staging of S / 2 + 2 symbols per region
    leave no room for a second wave in the LDS."""
    iz, io, sy = [-1], [-1], [0]

    def grow(v):
        a = len(iz)
        iz[v], io[v] = a, a + 1
        iz.extend([-1, -1]); io.extend([-1, -1]); sy.extend([0, 0])
        return [a, a + 1]

    l1 = grow(0)
    keep = grow(l1[0])[0]                                        # a leaf at depth 2, kept
    leaves = [x for x in range(len(iz)) if iz[x] < 0 and x != keep]
    while sum(z >= 0 for z in iz) < 127:
        leaves += grow(leaves.pop(0))                            # breadth first: the others at depths 7 and 8
    iz, io, sy = np.array(iz), np.array(io), np.array(sy)
    lv = np.flatnonzero(iz < 0)
    sy[lv] = np.arange(lv.size)
    sy = EC._tail_bytes(iz, sy)
    return iz, io, sy


def _tiny_reads(rng, lo, hi, count):
    """count reads of 1 to 3 bytes with sources anywhere in [lo, hi)."""
    lens = rng.integers(1, 4, count)
    return [(int(rng.integers(lo, hi - l + 1)), int(l)) for l in lens]


@pytest.mark.parametrize("kind", ["bible", "wave1"])
def test_stride_loops(hh, kind, monkeypatch):
    """3000 reads of 1 to 3 bytes in one block and exactly one read in
    another: a piece list far longer than a workgroup has threads, walked
    with the workgroup's stride every round -- for bible.txt's own code and
    for a tree that runs one wave, 64 threads, per workgroup."""
    import torch
    rng = np.random.default_rng(3000)
    if kind == "bible":
        text, tree, data, index = _bible(hh, 4096 * 8)
        B = 4096 * 8
        dec = hh.Decoder(0)
        dec.set_tree(tree)
    else:
        iz, io, sy = _wave1()
        L = EC._lengths(iz, io, sy)
        syms = np.array(sorted(L), np.uint8)
        p = np.array([2.0 ** -L[int(s)] for s in syms])
        B = 9000
        text = rng.choice(syms, size=4 * B + 100, p=p / p.sum()).astype(np.uint8)
        tree = hh.Tree(iz, io, sy)
        data, index = tree.encode_blocks(text, B)
        monkeypatch.setenv("HH_FSM_K", "7")                      # (read by set_tree)
        dec = hh.Decoder(0)
        dec.set_tree(tree)
        monkeypatch.delenv("HH_FSM_K")
        assert dec.batch_round_tiles() == 1 and dec.geometry()["K"] == 7, dec.geometry()
        assert int(index[2, 1]) > 2 * 64 * 256                   # (block 2: more than two rounds)
    try:
        n = text.size
        srcs = _tiny_reads(rng, 2 * B, 3 * B, 3000) + [(B // 2, 77)]
        reads, end = _pack(srcs, 3, rng)
        out, read_len, status, summ = _both(dec, torch.from_numpy(data).cuda(), _dev(index, 4), n, B, reads, end)
        assert not status.any() and np.array_equal(read_len, reads[:, 1])
        _exact(out, _want(out.size, reads, text))
        assert summ["total_len"] == end - 3
    finally:
        dec.close()


def test_block_scan(hh):
    """64-byte blocks, 5000 of them (the scan over the blocks takes five
    workgroups), reads in blocks 0, 1023, 1024, 1025 and the last only: the
    carries across the scan's workgroups and sparse walk ordinals."""
    import torch
    B, nb = 64, 5000
    text = np.fromfile(os.path.join(EC.FILES, "bible.txt"), np.uint8)[: B * nb - 11]
    n = text.size
    tree = hh.Tree.from_counts(np.bincount(text, minlength=256))
    data, index = tree.encode_blocks(text, B)
    assert index.shape[0] == nb
    srcs = []
    for b in (0, 1023, 1024, 1025, nb - 1):
        blen = min(B, n - b * B)
        srcs += [(b * B, 1), (b * B + 3, 20), (b * B + blen - 1, 1), (b * B + 10, blen - 10), (b * B + 30, 5)]
    srcs += [(1024 * B - 2, 4), (1024 * B - 1, B + 2)]          # (across the edges between the three neighbours)
    reads, end = _pack(srcs, 7, np.random.default_rng(64))
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        out, read_len, status, summ = _both(dec, torch.from_numpy(data).cuda(), _dev(index, 4), n, B, reads, end)
        assert not status.any() and np.array_equal(read_len, reads[:, 1])
        _exact(out, _want(out.size, reads, text))
        assert summ["total_len"] == end - 7 and summ["n_failed"] == 0
    finally:
        dec.close()


def test_failures_stay_local(hh):
    """An out-of-range read; a bad index entry under five reads (all five
    HH_ERR_ARG, their destinations untouched, a sixth read that only crosses
    into the block keeps its other part); every other read exact.  More than
    256 reads, with failures in the first, second and third result workgroup:
    the summary's count and first failure."""
    import torch
    B = 1000
    text, tree, data, index = _bible(hh, B)
    n = text.size
    DB = data.size
    idx = index.copy()
    idx[7, 0] |= 1                                              # block 7: off a 4-byte boundary
    idx[150, 0] = DB - 8                                        # block 150: its payload and pad pass data_bytes
    rng = np.random.default_rng(700)
    good = []
    while len(good) < 700:
        l = int(rng.integers(0, 300))
        s = int(rng.integers(0, n - l + 1))
        if not any(s // B <= b <= (s + max(l, 1) - 1) // B for b in (7, 150)):
            good.append((s, l))
    bad = {40: (n - 10, 11), 300: (7 * B + 5, 10), 301: (7 * B + 500, 100), 302: (7 * B, B), 303: (7 * B + 999, 1),
           304: (7 * B + 40, 3), 305: (6 * B + 990, 20), 600: (150 * B + 1, 50), 650: ((1 << 64) - 1, 2)}
    srcs = [bad[k] if k in bad else good.pop() for k in range(700)]
    reads, OB = _pack(srcs, 3)
    d_data = torch.cat([torch.from_numpy(data).cuda(), torch.zeros(4096, dtype=torch.uint8, device="cuda")])
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        out, read_len, status, summ = _both(dec, d_data, _dev(idx, 4), n, B, reads, OB, data_bytes=DB, out_bytes=OB)
        assert status.tolist() == [ERR_ARG if k in bad else 0 for k in range(700)]
        want = _want(out.size, reads, text, skip=tuple(k for k in bad if k != 305))
        d305 = int(reads[305, 2])
        want[d305 + 10: d305 + 20] = 0xAB                        # block 7's part of read 305
        _exact(out, want)
        exp = reads[:, 1].copy()
        exp[[k for k in bad]] = 0
        exp[305] = 10
        assert np.array_equal(read_len, exp)
        assert summ == {"total_len": int(sum(reads[k, 1] for k in range(700) if k not in bad)), "n_failed": len(bad),
                        "first_failed": 40, "first_status": ERR_ARG}
    finally:
        dec.close()


def test_short_block(hh):
    """Block 2's index entry says half its bits.  Of its pieces some lie
    before the stream's end (served), one across it (HH_ERR_FORMAT, the bytes
    there are delivered), some past it (HH_ERR_FORMAT, nothing); the
    neighbours' reads and the served ones are exact."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        S, W = dec.tile_bits() // 64, dec.batch_round_tiles()
        text, B, data, index = _five_blocks(name, W, S)
        n = text.size
        idx = index.copy()
        idx[2, 1] //= 2
        half = EC.oracle_prefix(E.any_code(name), data[int(idx[2, 0]):], int(idx[2, 1]))
        h = len(half)
        assert B // 4 + 100 < h < 3 * B // 4
        srcs = [(B + 5, B - 5), (2 * B + 10, B // 4 - 10), (2 * B + 3 * B // 4, B // 8), (2 * B + B // 8, B - B // 8),
                (3 * B, B), (2 * B + h - 1, 1), (2 * B + h, 1), (2 * B + h - 20, 40), (2 * B + 3, 5), (2 * B - 4, 30)]
        reads, end = _pack(srcs, 1)
        out, read_len, status, summ = _both(dec, torch.from_numpy(data).cuda(), _dev(idx, 4), n, B, reads, end)
        assert status.tolist() == [0, 0, ERR_FORMAT, ERR_FORMAT, 0, 0, ERR_FORMAT, ERR_FORMAT, 0, 0]
        got3 = h - B // 8
        assert read_len.tolist() == [B - 5, B // 4 - 10, 0, got3, B, 1, 0, 20, 5, 30]
        want = _want(out.size, reads, text, skip=(2, 3, 6, 7))
        d3, d7 = int(reads[3, 2]), int(reads[7, 2])
        want[d3: d3 + got3] = half[B // 8:]
        want[d7: d7 + 20] = half[h - 20:]
        want[int(reads[5, 2])] = half[h - 1]                     # (the tail rule's byte when the cut is inside a code)
        _exact(out, want)
        ok = [0, 1, 4, 5, 8, 9]
        assert summ == {"total_len": int(reads[ok, 1].sum()), "n_failed": 4, "first_failed": 2, "first_status": ERR_FORMAT}
    finally:
        dec.close()


def test_budget_overflow(hh):
    """test_gpu_batch_shapes.py::test_reads_past_the_budget's construction in
    small: destinations overlap (dst_off = src_off - c for one c, so every
    output byte has one possible value), and 60 four-piece reads exhaust the
    budget P = out_bytes / B + 2 m; the reads after that get HH_ERR_ARG unless
    they are empty.  Statuses as test_blocks_read.model()."""
    import torch
    B, k0 = 1000, 100
    text, tree, data, index = _bible(hh, B)
    n = text.size
    c, OB = k0 * B - 1, 4 * B + 500
    rng = np.random.default_rng(15)
    m = 122
    P = budget(OB, B, m)
    four = [(k * B - 1, 2 * B + 2) for k in rng.integers(k0, k0 + 3, 70).tolist()]
    two = [(k * B - a, a + b) for k, a, b in zip(rng.integers(k0 + 1, k0 + 5, 40).tolist(),
                                                 rng.integers(1, 401, 40).tolist(), rng.integers(1, 401, 40).tolist())]
    tail = [(k0 * B + 7, 0), (n - 10, 20), ((k0 + 2) * B - 3, 9), ((k0 + 1) * B + 5, 10), (n, 0), (k0 * B + 9, 1)]
    srcs = two[:20] + four + two[20:] + tail + tail
    reads = [(s, l, s - c if c <= s <= c + OB - l else 0) for s, l in srcs]
    assert len(reads) == m
    stat, first, pieces = model(reads, n, B, OB, P)
    assert ERR_ARG in stat and 0 in stat[stat.index(ERR_ARG):] and len(pieces) <= P < sum(
        (s + l - 1) // B - s // B + 1 for s, l, _ in reads if l and s + l <= n)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        out, read_len, status, summ = _both(dec, torch.from_numpy(data).cuda(), _dev(index, 4), n, B,
                                            np.array(reads, np.uint64), OB, out_bytes=OB)
        assert status.tolist() == stat
        assert read_len.tolist() == [0 if s else l for (_, l, _), s in zip(reads, stat)]
        want = np.full(out.size, 0xAB, np.uint8)
        for (s, l, d), st in zip(reads, stat):
            if not st:
                want[d: d + l] = text[s: s + l]
        _exact(out, want)
        assert summ == _summary(reads, np.array(stat))
    finally:
        dec.close()


def test_stream_ordered(hh):
    """Encoder.encode_blocks(..., items_out=t) and gather_blocks on the same
    side stream with nothing between them; then gather_blocks and read_blocks
    back to back on two streams (the workspace is one per decoder: the second
    waits for the first call's event).  One synchronise at the end."""
    import torch
    B = 4096
    text, tree, data, index = _bible(hh, B)
    n, nb = text.size, index.shape[0]
    rng = np.random.default_rng(8)
    srcs = [(int(rng.integers(0, n - 600)), int(rng.integers(0, 600))) for _ in range(400)]
    reads, end = _pack(srcs, 5, rng)
    reads2, end2 = _pack(srcs[::-1], 2, rng)
    enc, dec = hh.Encoder(0), hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_text = torch.from_numpy(text).cuda()
        buf = torch.zeros(hh.encode_blocks_bound(tree, n, B) + hh.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
        t = torch.full((nb, 4), -1, dtype=torch.int64, device="cuda")
        d_reads, d_reads2, d_index2 = _dev(reads, 3), _dev(reads2, 3), _dev(index, 4)
        d_data2 = torch.from_numpy(data).cuda()
        outs = [torch.full((e + GUARD,), 0xAB, dtype=torch.uint8, device="cuda") for e in (end, end2, end2)]
        rs = [_results(400) for _ in range(3)]
        torch.cuda.synchronize()
        with _two_streams(hh) as (s1, s2):
            enc.encode_blocks(tree, d_text, B, buf, stream=s1, items_out=t)
            dec.gather_blocks(buf, t, n, B, d_reads, outs[0], rs[0][0], rs[0][1], summary=rs[0][2], stream=s1)
            dec.gather_blocks(d_data2, d_index2, n, B, d_reads2, outs[1], rs[1][0], rs[1][1], summary=rs[1][2], stream=s2)
            dec.read_blocks(d_data2, d_index2, n, B, d_reads2, outs[2], rs[2][0], rs[2][1], summary=rs[2][2], stream=s1)
            torch.cuda.synchronize()
            dec.close()                                          # (while the streams its event was recorded on exist)
        for (read_len, status, summ), o, rd in zip(rs, outs, (reads, reads2, reads2)):
            assert not status.cpu().numpy().any()
            assert np.array_equal(read_len.cpu().numpy().astype(np.uint64), rd[:, 1])
            assert dec.batch_summary(summ) == {"total_len": int(rd[:, 1].sum()), "n_failed": 0, "first_failed": NONE,
                                               "first_status": 0}
            _exact(o.cpu().numpy(), _want(o.numel(), rd, text))
    finally:
        enc.close()
        dec.close()


def test_arguments(hh):
    """What the host can see is refused before anything is enqueued, the
    outputs untouched: null pointers, block_syms 0 (HH_ERR_ARG); a piece
    budget or a block count of 2^32 - 1 or more, computed and refused before
    anything is allocated (HH_ERR_UNSUPPORTED).  No reads: HH_OK and the empty
    summary; no symbols: the read of nothing is served."""
    import torch
    dec = _decoder(hh, "kjv")
    bare = hh.Decoder(0)
    try:
        L = hh.lib()
        data = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        out = torch.full((1024,), 0xAB, dtype=torch.uint8, device="cuda")
        index = _dev_items(np.array([[0, 256, 0, 0]], np.uint64))
        reads = _dev(np.array([[0, 4, 0]], np.uint64), 3)
        read_len = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def call(h, d=data.data_ptr(), ix=index.data_ptr(), n_syms=64, B=64, rd=reads.data_ptr(), m=1,
                 o=out.data_ptr(), ob=1024, rl=read_len.data_ptr(), s=status.data_ptr(), summ=None):
            return L.hh_decode_blocks_gather(h, d, 4096, ix, n_syms, B, rd, m, o, ob, rl, s, summ, st)

        assert call(None) == ERR_ARG
        assert call(bare._h) == ERR_ARG                          # no tree
        for kw in ({"d": None}, {"ix": None}, {"rd": None}, {"o": None}, {"rl": None}, {"s": None}, {"B": 0},
                   {"d": data.data_ptr() + 1}):
            assert call(dec._h, **kw) == ERR_ARG, kw
        lim = 2 ** 32 - 1
        # the budget P = out_bytes / block_syms + 2 m
        assert budget(2 ** 40, 1, 1) is None and budget(lim - 2, 1, 1) is None and budget(lim - 3, 1, 1) == lim - 1
        assert call(dec._h, ob=2 ** 40, B=1) == ERR_UNSUPPORTED
        assert call(dec._h, ob=lim - 2, B=1) == ERR_UNSUPPORTED
        # the blocks nb = ceil(n_syms / block_syms): 2^32 - 1 is refused (a workspace for it cannot be had: an
        # attempt would come back as HH_ERR_NOMEM), and it is the gathered call's check alone
        assert -(-(2 * lim - 1) // 2) == lim and -(-(2 * lim - 2) // 2) == lim - 1
        assert call(dec._h, n_syms=lim, B=1) == ERR_UNSUPPORTED
        assert call(dec._h, n_syms=2 * lim - 1, B=2) == ERR_UNSUPPORTED
        assert call(dec._h, n_syms=2 ** 64 - 1, B=2 ** 31) == ERR_UNSUPPORTED
        with pytest.raises(hh.HipHuffError) as e:
            dec.gather_blocks(data, _dev_items(np.zeros((64, 4), np.uint64)), 64, 1, reads, out, read_len, status,
                              out_bytes=2 ** 40)
        assert e.value.status == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _clean(out) and read_len.item() == 77 and status.item() == 77
        # no symbols: a null index is fine, the read of nothing at 0 is served and a read of something is out of range
        two = _dev(np.array([[0, 0, 5], [0, 1, 5]], np.uint64), 3)
        rl2 = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        s2 = torch.full((2,), 77, dtype=torch.int32, device="cuda")
        summ = torch.full((6,), 77, dtype=torch.int32, device="cuda")
        assert call(dec._h, ix=None, n_syms=0, rd=two.data_ptr(), m=2, rl=rl2.data_ptr(), s=s2.data_ptr(),
                    summ=summ.data_ptr()) == 0
        torch.cuda.synchronize()
        assert rl2.tolist() == [0, 0] and s2.tolist() == [0, ERR_ARG] and _clean(out)
        assert dec.batch_summary(summ) == {"total_len": 0, "n_failed": 1, "first_failed": 1, "first_status": ERR_ARG}
        for d in (dec, bare):
            n, s, summ = d.gather_blocks(data, index, 64, 64, np.zeros((0, 3), np.uint64), out, summary=True)
            torch.cuda.synchronize()
            assert n.numel() == 0 and s.numel() == 0
            assert d.batch_summary(summ) == {"total_len": 0, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        assert _clean(out)
    finally:
        dec.close()
        bare.close()
