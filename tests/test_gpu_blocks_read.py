"""Range reads over a block-coded buffer (hh_decode_blocks_read,
Decoder.read_blocks; csrc/hh_batch_read.hip around the windowed k_batch) on
the GPU: byte ranges of the uncompressed data, each delivered to its own
destination by one stream-ordered call.  tests/test_blocks_read.py runs the
same rules and windows on the host (the overflow corners of the read rules
are tested there only).

As in tests/test_gpu_batch.py every output is 0xAB first and compared whole,
the bytes no read may write included; the reference of a read is the slice of
the text the blocks were encoded from."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import edge_cases as E
from test_blocks_read import block_windows, round_counts, rounds_for
from test_gpu_batch import GUARD, _clean, _decoder, _two_streams
from test_gpu_batch_items import _page_locked, _results

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FORMAT, ERR_UNSUPPORTED = -1, -3, -10
NONE = 0xffffffff
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _drop_buffers():
    yield
    import torch
    _blocked.cache_clear()
    _bible.cache_clear()
    torch.cuda.empty_cache()


def _dev(a, cols):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64).reshape(-1, cols)).cuda()


@functools.lru_cache(maxsize=None)
def _blocked(name, W, S):
    """Five blocks of code `name`, each a little over three rounds of W tiles
    of 64 S bits, the last one short: (text, block_syms, payload + pad,
    index rows) from the host encoder."""
    c = E.code(name)
    L = E._lengths(c.izero, c.ione, c.sym)
    rng = np.random.default_rng([W, S, E.CODE_NAMES.index(name)])
    if c.probs is None:
        syms, p = np.array(sorted(L), np.uint8), None
    else:
        syms, p = c.probs
    RB = 64 * W * S
    draw = lambda n: rng.choice(syms, size=n, p=p).astype(np.uint8)
    avg = float(np.mean([L[int(s)] for s in draw(20000)]))
    B = int(3.3 * RB / avg)
    text = draw(4 * B + B // 3)
    data, index = c.tree().encode_blocks(text, B)
    assert index.shape[0] == 5 and all(3 * RB < b < 4 * RB for b in index[:4, 1].tolist()), (index, RB)
    return text, B, data, index


@functools.lru_cache(maxsize=None)
def _bible(hh_mod, B):
    """The first 256 KiB of files/bible.txt in blocks of B under its own
    Huffman code: (text, tree, payload + pad, index rows)."""
    text = np.fromfile(os.path.join(E.FILES, "bible.txt"), np.uint8)[: 256 * 1024]
    tree = hh_mod.Tree.from_counts(np.bincount(text, minlength=256))
    data, index = tree.encode_blocks(text, B)
    return text, tree, data, index


def _pack(srcs, start, rng=None):
    """reads (src_off, len, dst_off) for the (src_off, len) of srcs, the
    destinations packed without gaps from `start`, in shuffled order when rng
    is given; the end offset."""
    order = rng.permutation(len(srcs)) if rng is not None else np.arange(len(srcs))
    reads, off = np.zeros((len(srcs), 3), np.uint64), start
    for k in order:
        reads[k] = (srcs[k][0], srcs[k][1], off)
        off += srcs[k][1]
    return reads, off


def _want(size, reads, text, skip=()):
    want = np.full(size, 0xAB, np.uint8)
    for k, (s, l, d) in enumerate(reads.tolist()):
        if k not in skip:
            want[d: d + l] = text[s: s + l]
    return want


def _same(out, want):
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"byte {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}; {bad.size} bytes differ"


def _run(dec, d_data, d_index, n_syms, B, reads, out, **kw):
    """One call, waited for: (read_len, status, summary dict)."""
    import torch
    d_reads = reads if torch.is_tensor(reads) else _dev(reads, 3)
    read_len, status, summ = dec.read_blocks(d_data, d_index, n_syms, B, d_reads, out, summary=True, **kw)
    torch.cuda.synchronize()
    return read_len.cpu().numpy().astype(np.uint64), status.cpu().numpy(), dec.batch_summary(summ)


@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_window_edges(hh, name):
    """Five blocks of a little over three rounds, the last short.  In block 1
    the windows of tests/test_blocks_read.py around every round boundary, the
    empty window and the whole block; reads across one and two block edges,
    the whole buffer, an empty read at n_syms.  Destinations back to back
    from offset 1 in shuffled order: the whole output is the slices, every
    status 0, the summary the sum, the stats zero but state_machine 3."""
    import torch
    dec = _decoder(hh, name)
    try:
        S, W = dec.tile_bits() // 64, dec.batch_round_tiles()
        text, B, data, index = _blocked(name, W, S)
        n = text.size
        c = E.code(name)
        blk = data[int(index[1, 0]):]
        bits = int(index[1, 1])
        cs = round_counts(c, blk, bits, 64 * W * S, text[B: 2 * B])
        assert len(cs) == 3 and 0 < cs[0] < cs[2] < B
        assert rounds_for(cs, cs[0] - 1, 1) == 1 and rounds_for(cs, cs[0], 1) == 2     # (what the windows are about)
        srcs = [(B + s, l) for s, l in block_windows(cs, B)]
        srcs += [(B - 1, 2), (B - 1, B + 2), (0, n), (n, 0), (n - 1, 1), (4 * B - 1, n - 4 * B + 1)]
        reads, end = _pack(srcs, 1, np.random.default_rng(5))
        d_data, d_index = torch.from_numpy(data).cuda(), _dev(index, 4)
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        read_len, status, summ = _run(dec, d_data, d_index, n, B, reads, out)
        st = dec.stats()
        assert not status.any(), status
        assert np.array_equal(read_len, reads[:, 1])
        _same(out, _want(out.numel(), reads, text))
        assert summ == {"total_len": end - 1, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        assert st.pop("state_machine") == 3 and not any(st.values()), st
    finally:
        dec.close()


@pytest.mark.parametrize("B", [1000, 4096])
def test_random_reads(hh, B):
    """2000 reads of 0 .. 3 B bytes anywhere in 256 KiB of bible.txt, the
    destinations a random permutation packed without gaps."""
    import torch
    text, tree, data, index = _bible(hh, B)
    n = text.size
    rng = np.random.default_rng(2000 + B)
    lens = rng.integers(0, 3 * B + 1, 2000)
    srcs = [(int(rng.integers(0, n - l + 1)), int(l)) for l in lens]
    reads, end = _pack(srcs, 0, rng)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_data, d_index = torch.from_numpy(data).cuda(), _dev(index, 4)
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        read_len, status, summ = _run(dec, d_data, d_index, n, B, reads, out)
        assert not status.any() and np.array_equal(read_len, reads[:, 1])
        _same(out, _want(out.numel(), reads, text))
        assert summ == {"total_len": int(lens.sum()), "n_failed": 0, "first_failed": NONE, "first_status": 0}
    finally:
        dec.close()


def test_whole_buffer_equals_full_decode(hh):
    """One read [0, n_syms) gives the bytes decode_batch_items gives with the
    same index."""
    import torch
    text, tree, data, index = _bible(hh, 4096)
    n = text.size
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_data, d_index = torch.from_numpy(data).cuda(), _dev(index, 4)
        full = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status = dec.decode_batch_items(d_data, d_index, full)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any() and int(out_len.sum()) == n
        out = torch.full_like(full, 0xAB)
        read_len, status, summ = _run(dec, d_data, d_index, n, 4096, np.array([[0, n, 0]], np.uint64), out)
        assert status.tolist() == [0] and read_len.tolist() == [n] and summ["total_len"] == n
        assert torch.equal(out, full) and _clean(out[n:])
        assert np.array_equal(out[:n].cpu().numpy(), text)
    finally:
        dec.close()


def test_bad_reads_fail_alone(hh):
    """Among good reads: a source and a destination out of range, a read
    whose end wraps past 2^64, a read through an index entry with an odd
    data_off and one through an entry whose payload passes data_bytes.
    data_bytes and out_bytes are declared smaller than the tensors, so every
    bad offset still lies inside the allocations and the 0xAB shows any
    write.  The rangeless reads deliver nothing; of the reads through a bad
    entry only that block's part is missing; the good reads are exact."""
    import torch
    B = 1000
    text, tree, data, index = _bible(hh, B)
    n = text.size
    DB = data.size
    idx = index.copy()
    idx[7, 0] |= 1                                              # block 7: off a 4-byte boundary
    idx[20, 0] = DB - 8                                         # block 20: its payload and pad pass data_bytes
    rng = np.random.default_rng(77)
    good = []
    while len(good) < 60:
        l = int(rng.integers(0, 2 * B))
        s = int(rng.integers(0, n - l + 1))
        if not any(s // B <= b <= (s + max(l, 1) - 1) // B for b in (7, 20)):
            good.append((s, l))
    bad = {5: (n - 10, 11), 11: (100, 500), 17: (M64, 2), 23: (6 * B + 500, 2 * B), 31: (20 * B + 1, B - 2),
           40: (19 * B + 990, 20)}
    srcs = []
    for k in range(66):
        srcs.append(bad[k] if k in bad else good.pop())
    reads, OB = _pack(srcs, 3)
    reads[11, 2] = OB - 499                                      # read 11's destination reaches past out_bytes
    d_data = torch.cat([torch.from_numpy(data).cuda(), torch.zeros(4096, dtype=torch.uint8, device="cuda")])
    out = torch.full((OB + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        read_len, status, summ = _run(dec, d_data, _dev(idx, 4), n, B, reads, out, data_bytes=DB, out_bytes=OB)
        assert status.tolist() == [ERR_ARG if k in bad else 0 for k in range(66)]
        want = _want(out.numel(), reads, text, skip=(5, 11, 17))
        # the bad blocks' parts stay untouched
        for k, b in ((23, 7), (31, 20), (40, 20)):
            s, l, d = reads[k].tolist()
            lo, hi = max(s, b * B), min(s + l, (b + 1) * B)
            want[d + lo - s: d + hi - s] = 0xAB
        _same(out, want)
        exp_len = reads[:, 1].copy()
        exp_len[[5, 11, 17]] = 0
        exp_len[23] = 2 * B - B                                  # blocks 6 and 8 delivered, block 7 not
        exp_len[31] = 0
        exp_len[40] = 10                                         # block 19's ten bytes
        assert np.array_equal(read_len, exp_len)
        assert summ == {"total_len": int(sum(reads[k, 1] for k in range(66) if k not in bad)), "n_failed": 6,
                        "first_failed": 5, "first_status": ERR_ARG}
    finally:
        dec.close()


def test_short_block_is_format_error(hh):
    """Block 2's index entry says half its bits: a read inside the block's
    first quarter is served, a read in its last quarter is HH_ERR_FORMAT with
    nothing delivered, one from the first quarter to the end delivers what
    the half stream holds and nothing past it; the neighbours' reads are
    exact."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        S, W = dec.tile_bits() // 64, dec.batch_round_tiles()
        text, B, data, index = _blocked(name, W, S)
        n = text.size
        idx = index.copy()
        idx[2, 1] //= 2
        half = E.oracle_prefix(E.code(name), data[int(idx[2, 0]):], int(idx[2, 1]))
        assert B // 4 + 100 < len(half) < 3 * B // 4
        srcs = [(B + 5, B - 5), (2 * B + 10, B // 4 - 10), (2 * B + 3 * B // 4, B // 8), (2 * B + B // 8, B - B // 8),
                (3 * B, B), (B + B // 2, B // 2)]
        reads, end = _pack(srcs, 1)
        d_data = torch.from_numpy(data).cuda()
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        read_len, status, summ = _run(dec, d_data, _dev(idx, 4), n, B, reads, out)
        assert status.tolist() == [0, 0, ERR_FORMAT, ERR_FORMAT, 0, 0]
        got3 = len(half) - B // 8
        assert read_len.tolist() == [B - 5, B // 4 - 10, 0, got3, B, B // 2] and got3 < srcs[3][1]
        want = _want(out.numel(), reads, text, skip=(2, 3))
        d3 = int(reads[3, 2])
        want[d3: d3 + got3] = half[B // 8:]
        _same(out, want)
        ok = [0, 1, 4, 5]
        assert summ == {"total_len": int(reads[ok, 1].sum()), "n_failed": 2, "first_failed": 2,
                        "first_status": ERR_FORMAT}
    finally:
        dec.close()


def test_stream_ordered(hh):
    """On a side stream the reads and the index come up from page-locked
    memory by asynchronous copies queued immediately before the call, with no
    synchronisation in between; a second call on another stream follows at
    once (the workspace is one per decoder: it waits for the first call's
    event).  One synchronise at the end, then both are right."""
    import torch
    B = 4096
    text, tree, data, index = _bible(hh, B)
    n = text.size
    rng = np.random.default_rng(6)
    srcs = [(int(rng.integers(0, n - 3 * B)), int(rng.integers(0, 3 * B))) for _ in range(300)]
    reads, end = _pack(srcs, 5, rng)
    reads2, end2 = _pack(srcs[::-1], 2, rng)
    ireads = np.ascontiguousarray(reads).view(np.int64)
    iindex = np.ascontiguousarray(index).view(np.int64)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        d_data = torch.from_numpy(data).cuda()
        d_index2, d_reads2 = _dev(index, 4), _dev(reads2, 3)
        d_reads = torch.zeros((300, 3), dtype=torch.int64, device="cuda")
        d_index = torch.zeros((index.shape[0], 4), dtype=torch.int64, device="cuda")
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out2 = torch.full((end2 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        r1, r2 = _results(300), _results(300)
        hip = hh.lib()
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        torch.cuda.synchronize()
        with _page_locked(hh, ireads) as h_reads, _page_locked(hh, iindex) as h_index, _two_streams(hh) as (s1, s2):
            assert hip.hipMemcpyAsync(d_reads.data_ptr(), h_reads, ireads.nbytes, 1, s1.cuda_stream) == 0
            assert hip.hipMemcpyAsync(d_index.data_ptr(), h_index, iindex.nbytes, 1, s1.cuda_stream) == 0
            dec.read_blocks(d_data, d_index, n, B, d_reads, out, r1[0], r1[1], summary=r1[2], stream=s1)
            dec.read_blocks(d_data, d_index2, n, B, d_reads2, out2, r2[0], r2[1], summary=r2[2], stream=s2)
            torch.cuda.synchronize()
            dec.close()                                          # (while the streams its event was recorded on exist)
        for (read_len, status, summ), o, rd in ((r1, out, reads), (r2, out2, reads2)):
            assert not status.cpu().numpy().any()
            assert np.array_equal(read_len.cpu().numpy().astype(np.uint64), rd[:, 1])
            assert dec.batch_summary(summ) == {"total_len": int(rd[:, 1].sum()), "n_failed": 0, "first_failed": NONE,
                                               "first_status": 0}
            _same(o, _want(o.numel(), rd, text))
    finally:
        dec.close()


def test_producer_to_reader(hh):
    """Encoder.compress_blocks(..., items_out=t) leaves the index on the
    device; read_blocks takes t as it is, with no host copy of it."""
    import torch
    text = np.fromfile(os.path.join(E.FILES, "bible.txt"), np.uint8)[: 100 * 1000 + 123]
    n, Bs = text.size, 1000
    nb = -(-n // Bs)
    d_text = torch.from_numpy(text).cuda()
    enc, dec = hh.Encoder(0), hh.Decoder(0)
    try:
        cap = hh.compress_blocks_bound(n, Bs)
        buf = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        t = torch.full((nb, 4), -1, dtype=torch.int64, device="cuda")
        ctree, _, total = enc.compress_blocks(d_text, Bs, buf[:cap], items_out=t)
        dec.set_tree(ctree)
        rng = np.random.default_rng(7)
        srcs = [(int(rng.integers(0, n - 2500)), int(rng.integers(0, 2500))) for _ in range(200)] + [(n - 123, 123), (0, n)]
        reads, end = _pack(srcs, 1, rng)
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        # (a host array of reads: uploaded on the call's stream)
        read_len, status, summ = dec.read_blocks(buf[: total + hh.PAYLOAD_PAD], t, n, Bs, reads, out, summary=True)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any() and dec.batch_summary(summ)["total_len"] == end - 1
        _same(out, _want(out.numel(), reads, text))
    finally:
        enc.close()
        dec.close()


def test_arguments(hh):
    """What the host can see is refused before anything is enqueued, the
    outputs untouched: no tree, null pointers, a null index with n_syms > 0,
    block_syms 0, d_data off a 4-byte boundary (HH_ERR_ARG); a tree the batch
    cannot take and a piece budget of 2^32 - 1 or more, before any allocation
    (HH_ERR_UNSUPPORTED).  No reads: HH_OK and the empty summary."""
    import torch
    from test_gpu_batch_items import _dev_items
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
            return L.hh_decode_blocks_read(h, d, 4096, ix, n_syms, B, rd, m, o, ob, rl, s, summ, st)

        assert call(None) == ERR_ARG
        assert call(bare._h) == ERR_ARG                          # no tree
        for kw in ({"d": None}, {"ix": None}, {"rd": None}, {"o": None}, {"rl": None}, {"s": None}, {"B": 0},
                   {"d": data.data_ptr() + 1}):
            assert call(dec._h, **kw) == ERR_ARG, kw
        with pytest.raises(hh.HipHuffError) as e:
            dec.read_blocks(data[1:], index, 64, 64, reads, out, read_len, status)
        assert e.value.status == ERR_ARG
        # the budget: out_bytes / block_syms + 2 m >= 2^32 - 1, refused before anything is allocated or enqueued
        # (a workspace for 2^40 slots cannot be had: an attempt would come back as HH_ERR_NOMEM)
        assert call(dec._h, ob=2 ** 40, B=1) == ERR_UNSUPPORTED
        assert call(dec._h, ob=2 ** 32 - 3, B=1) == ERR_UNSUPPORTED      # P = 2^32 - 1 exactly
        with pytest.raises(hh.HipHuffError) as e:
            dec.read_blocks(data, _dev_items(np.zeros((64, 4), np.uint64)), 64, 1, reads, out, read_len, status,
                            out_bytes=2 ** 40)
        assert e.value.status == ERR_UNSUPPORTED
        # a tree past the state machine (test_gpu_batch_items.py::test_host_checked_arguments')
        rng = np.random.default_rng(96)
        izl, iol, leaves = [-1], [-1], [0]
        while len(leaves) < 300:
            v = leaves.pop(int(rng.integers(len(leaves))))
            a = len(izl)
            izl[v], iol[v] = a, a + 1
            izl += [-1, -1]
            iol += [-1, -1]
            leaves += [a, a + 1]
        rz = np.array(izl)
        rs = rng.integers(0, 256, size=len(rz)).astype(np.uint8)
        rs[rz != -1] = 0
        dec.set_tree(hh.Tree(rz, np.array(iol), rs))
        assert call(dec._h) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _clean(out) and read_len.item() == 77 and status.item() == 77
        # a null index is fine when there are no symbols: the read of nothing at 0 is served
        dec.set_tree(E.code("kjv").tree())
        empty = _dev(np.array([[0, 0, 5]], np.uint64), 3)
        assert call(dec._h, ix=None, n_syms=0, rd=empty.data_ptr()) == 0
        torch.cuda.synchronize()
        assert read_len.item() == 0 and status.item() == 0 and _clean(out)
        for d in (dec, bare):
            n, s, summ = d.read_blocks(data, index, 64, 64, np.zeros((0, 3), np.uint64), out, summary=True)
            torch.cuda.synchronize()
            assert n.numel() == 0 and s.numel() == 0
            assert d.batch_summary(summ) == {"total_len": 0, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        assert _clean(out)
    finally:
        dec.close()
        bare.close()
