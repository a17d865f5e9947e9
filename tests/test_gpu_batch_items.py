"""The batched decode from a device-resident item list
(hh_decode_batch_device_items; csrc/hh_batch_plan.hip around k_batch) on the
GPU: the same decode as hh_decode_batch_device stream for stream, with the
items checked and ordered, and the results delivered, by kernels on the
caller's stream.  tests/test_batch_plan.py runs the plan's rules on the host
(the overflow corners of the validity rule are tested there only).

As in tests/test_gpu_batch.py every output is 0xAB first and compared byte
for byte, the bytes no stream may write included.  Side streams come from
its _two_streams (tests/test_gpu_stream_order.py says why)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import edge_cases as E
import test_gpu_batch as B
from test_emu_batch import batch_cuts
from test_encode_blocks import strain_text
from test_gpu_batch import GUARD, _check_exact, _clean, _decoder, _packed, _refs, _two_streams
from test_gpu_encode import _random_tree

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -5, -10
NONE = 0xffffffff


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _drop_refs():
    yield
    import torch
    B._REFS.clear()
    torch.cuda.empty_cache()


def _dev_items(items):
    import torch
    return torch.from_numpy(np.ascontiguousarray(items, np.uint64).view(np.int64).reshape(-1, 4)).cuda()


def _results(n):
    """(out_len, status, summary) tensors for a batch on a side stream, made
    on the default stream beforehand: nothing of torch's is then allocated in
    the pool of a stream that _two_streams destroys."""
    import torch
    return (torch.full((n,), -7, dtype=torch.int64, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            torch.full((6,), -7, dtype=torch.int32, device="cuda"))


@contextlib.contextmanager
def _page_locked(hh, arr):
    """The address of a page-locked copy of arr, this test's own
    (hipHostMalloc through the runtime libhiphuff.so runs on, freed
    afterwards).  Not torch's pin_memory(): its allocator notes the stream of
    a non-blocking copy in the block and records an event on that stream when
    the tensor is freed -- here after _two_streams has destroyed the stream."""
    hip = hh.lib()
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipHostMalloc(C.byref(p), arr.nbytes, 0) == 0
    try:
        C.memmove(p.value, arr.ctypes.data, arr.nbytes)
        yield p.value
    finally:
        hip.hipHostFree(p)


def _run(dec, d_data, items, out, stream=None, **kw):
    """One items batch, waited for: (out_len uint64[n], status int32[n], summary dict)."""
    import torch
    out_len, status, summ = dec.decode_batch_items(d_data, _dev_items(items), out, summary=True, stream=stream, **kw)
    torch.cuda.synchronize()
    return out_len.cpu().numpy().astype(np.uint64), status.cpu().numpy(), dec.batch_summary(summ)


@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_breakpoints(hh, name):
    """test_gpu_batch.py::test_breakpoints' batch (every length at which a
    stream's rounds change shape, outputs back to back from offset 1 with
    exact capacities) from a device list: lengths and bytes are the oracle's,
    every status 0, the summary the sum; hh_decode_batch_device of the same
    batch gives the same out, out_len and status; the stats are zero but for
    state_machine 3."""
    import torch
    dec = _decoder(hh, name)
    try:
        S = dec.tile_bits() // 64
        W = dec.batch_round_tiles()
        data, bits, _ = E.stream(name, S, 49)
        cuts = batch_cuts(S, W, dec._tree.info()["maxlen"], bits)
        keys = [(0, b) for b in cuts]
        refs = _refs(name, data, keys)
        items, end = _packed(keys, refs, 1)
        d_data = torch.from_numpy(data).cuda()
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status, summ = _run(dec, d_data, items, out)
        st = dec.stats()
        assert not status.any(), status
        _check_exact(out, items, refs, out_len)
        assert _clean(out[:1]) and _clean(out[end:])
        assert summ == {"total_len": sum(len(r) for r in refs), "n_failed": 0, "first_failed": NONE,
                        "first_status": 0}
        assert st.pop("state_machine") == 3 and not any(st.values()), st
        out2 = torch.full_like(out, 0xAB)
        out_len2, status2 = dec.decode_batch(d_data, items, out2)
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and np.array_equal(out_len, out_len2) and np.array_equal(status, status2)
    finally:
        dec.close()


def test_more_streams_than_workgroups_mixed_lengths(hh):
    """About 600 streams of kjv: empty ones, 1 .. 3 S bits at seven word
    offsets, half a round to three rounds, and one of 64 rounds, past the
    plan's clamp of 63 (it is compared with hh_decode_device of that stream
    alone, the others with the oracle) -- more streams than resident
    workgroups, in every bin the plan has up to three and in its last.  The
    list in increasing, decreasing and shuffled order of length: all three
    outputs are byte-identical."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        S = dec.tile_bits() // 64
        W = dec.batch_round_tiles()
        RB = 64 * W * S
        data, bits, text = E.stream(name, S, 49)
        assert bits >= 3 * RB
        tree = dec._tree
        big, big_bits = tree.encode(np.tile(text, 64 * RB // bits + 2))
        keep = 63 * RB + 5 * S + 3
        assert big_bits > keep
        at = (data.size + 3) // 4 * 4
        both = np.zeros(at + (keep + 7) // 8 + 64, np.uint8)
        both[: data.size] = data
        both[at: at + (keep + 7) // 8] = big[: (keep + 7) // 8]
        d_data = torch.from_numpy(both).cuda()
        keys = [(4 * (k % 7), 0) for k in range(5)]
        keys += [(4 * (k % 7), 1 + (k * 3 * S) // 400) for k in range(400)]
        keys += [(0, RB // 2 + k * (5 * RB // 2) // 190 + k % 3) for k in range(190)]
        assert max(b for _, b in keys) <= 3 * RB + 2 and len(set(keys)) > 580
        refs = _refs(name, data, keys)
        one = torch.empty(keep // 2 + 64, dtype=torch.uint8, device="cuda")
        n_big = dec.decode_device(d_data[at:], keep, one)
        keys.append((at, keep))
        refs.append(one[:n_big].cpu().numpy())
        items, end = _packed(keys, refs, 3)
        n = len(keys)
        rng = np.random.default_rng(600)
        by_len = np.argsort(items[:, 1].astype(np.int64), kind="stable")
        outs = []
        for perm in (by_len, by_len[::-1], rng.permutation(n)):
            out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
            out_len, status, summ = _run(dec, d_data, items[perm], out)
            assert not status.any() and summ["n_failed"] == 0 and summ["total_len"] == end - 3
            _check_exact(out, items[perm], [refs[i] for i in perm], out_len)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    finally:
        dec.close()


def test_failures_are_per_stream(hh):
    """Capacity: every third stream with cap = len - 1 and one with cap 0,
    as test_gpu_batch.py::test_capacity_is_per_stream: HH_ERR_CAPACITY, the
    full out_len, nothing at or beyond out_off + cap.  Invalid items among
    good ones -- a data_off off a 4-byte boundary, payloads reaching past
    data_bytes, outputs reaching past out_bytes -- get HH_ERR_ARG and length
    0 while the good ones are exact: data_bytes and out_bytes are declared
    smaller than the tensors are, so every bad offset still lies inside the
    allocation and the 0xAB around shows any write.  The summary counts the
    failures and names the first."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        S = dec.tile_bits() // 64
        W = dec.batch_round_tiles()
        data, bits, _ = E.stream(name, S, 49)
        d_data = torch.from_numpy(data).cuda()
        cuts = batch_cuts(S, W, dec._tree.info()["maxlen"], bits)
        keys = [(0, b) for b in cuts]
        refs = _refs(name, data, keys)
        zero = len(cuts) - 2
        short = lambda k: k % 3 == 1 or k == zero
        items, end = _packed(keys, refs, 3, gap=64, cap=lambda k, n: 0 if k == zero else n - 1 if short(k) else n)
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status, summ = _run(dec, d_data, items, out)
        assert status.tolist() == [ERR_CAPACITY if short(k) else 0 for k in range(len(cuts))]
        _check_exact(out, items, refs, out_len)
        assert summ == {"total_len": sum(len(r) for r in refs), "n_failed": sum(short(k) for k in range(len(cuts))),
                        "first_failed": 1, "first_status": ERR_CAPACITY}
        # invalid items: the good streams are the cuts up to two tiles
        good = [(0, b) for b in cuts if b <= 2 * 64 * S + S + 1]
        DB = ((good[-1][1] + 7) // 8 + 64 + 3) // 4 * 4 + 256
        assert DB + 4096 < data.size
        bad_data = [(2, 256), (DB - 64, 8), (0, 8 * (DB - 64) + 1), (DB, 32), (DB + 1024, 32)]
        keys, isbad = [], []
        for k, g in enumerate(good):
            if k % 5 == 2 and bad_data:
                keys.append(bad_data.pop())
                isbad.append(True)
            keys.append(g)
            isbad.append(False)
        assert not bad_data and isbad.index(True) == 2
        grefs = iter(_refs(name, data, good))
        refs = [np.zeros(0, np.uint8) if b else next(grefs) for b in isbad]
        items, OB = _packed(keys, refs, 5, gap=16, cap=lambda k, n: 16 if isbad[k] else n)
        # outputs past out_bytes: three good streams' offsets and capacities replaced
        for k, (o, c) in zip((9, 15, len(keys) - 1), ((OB - 10, 11), (OB + 1, 0), (OB + 100, 50))):
            assert not isbad[k]
            isbad[k] = True
            refs[k] = np.zeros(0, np.uint8)
            items[k, 2], items[k, 3] = o, c
        out = torch.full((OB + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status, summ = _run(dec, d_data, items, out, data_bytes=DB, out_bytes=OB)
        assert status.tolist() == [ERR_ARG if b else 0 for b in isbad]
        _check_exact(out, items, refs, out_len)                  # (length 0 and 0xAB for the bad ones)
        assert _clean(out[OB:])
        assert summ == {"total_len": sum(len(r) for r in refs), "n_failed": sum(isbad), "first_failed": 2,
                        "first_status": ERR_ARG}
    finally:
        dec.close()


def test_stream_order(hh):
    """On a side stream, with no host wait between the steps: the items come
    up from pinned memory by a non-blocking copy, device ops on the same
    stream produce the payload, the items call follows; a second batch on the
    other stream and the same decoder (the workspace is one per decoder: it
    waits for the first batch's event).  One synchronise per stream, then both
    results are right."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        data, _, _ = E.stream(name, S, 49)
        keys = [(4 * k, 3 * TB + 11 * k) for k in range(1, 40)]
        refs = _refs(name, data, keys)
        items, end = _packed(keys, refs, 7)
        items2, end2 = _packed(keys[::-1], refs[::-1], 2)
        src = torch.from_numpy(data).cuda()
        d_items2 = _dev_items(items2)
        out = torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out2 = torch.full((end2 + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        d_items = torch.zeros((len(keys), 4), dtype=torch.int64, device="cuda")
        d_data = torch.zeros_like(src)
        tmp = torch.zeros_like(src)
        r1, r2 = _results(len(keys)), _results(len(keys))
        hip = hh.lib()
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        torch.cuda.synchronize()
        with _page_locked(hh, items) as h_items, _two_streams(hh) as (s1, s2):
            assert hip.hipMemcpyAsync(d_items.data_ptr(), h_items, items.nbytes, 1, s1.cuda_stream) == 0   # host to device
            with torch.cuda.stream(s1):
                for _ in range(3):                               # (work queued ahead of the batch)
                    tmp.copy_(src)
                    tmp.add_(1)
                torch.sub(tmp, 1, out=d_data)
            dec.decode_batch_items(d_data, d_items, out, *r1, stream=s1)
            dec.decode_batch_items(src, d_items2, out2, *r2, stream=s2)
            s1.synchronize()
            s2.synchronize()
            dec.close()                                          # (while the streams its event was recorded on exist)
        for (out_len, status, summ), o, it, rf in ((r1, out, items, refs), (r2, out2, items2, refs[::-1])):
            assert not status.cpu().numpy().any() and dec.batch_summary(summ)["n_failed"] == 0
            _check_exact(o, it, rf, out_len.cpu().numpy())
    finally:
        dec.close()


def test_with_other_calls(hh):
    """An items batch and, at once, set_tree to another code: the batch's
    output is the first tree's.  An items batch, then hh_decode_batch_device
    on another stream: both right.  An items batch while an
    hh_decode_device_async is pending: the pending decode is not checked by
    the call (its length is filled by wait() only), both are right and wait()
    is clean."""
    import torch
    name = "kjv"
    dec = _decoder(hh, name)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        data, _, _ = E.stream(name, S, 49)
        long_bits = 40 * TB + 17
        keys = [(0, long_bits)] + [(4 * k, 3 * TB + 11 * k) for k in range(1, 40)]
        refs = _refs(name, data, keys)
        d_data = torch.from_numpy(data).cuda()
        items, end = _packed(keys[1:], refs[1:], 7)
        d_items = _dev_items(items)
        fresh = lambda: torch.full((end + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_a, out_b, out_c, out_d = fresh(), fresh(), fresh(), fresh()
        one = torch.full((len(refs[0]) + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        n = len(keys) - 1
        ra, rb, rd = _results(n)[:2], _results(n)[:2], _results(n)[:2]
        torch.cuda.synchronize()
        with _two_streams(hh) as (s1, s2):
            dec.decode_batch_items(d_data, d_items, out_a, *ra, stream=s1)
            dec.set_tree(E.code("byte256").tree())
            s1.synchronize()
            dec.set_tree(E.code(name).tree())
            dec.decode_batch_items(d_data, d_items, out_b, *rb, stream=s1)
            len_c, st_c = dec.decode_batch(d_data, items, out_c, stream=s2)
            s1.synchronize()
            n1 = dec.decode_device_async(d_data, long_bits, one[: len(refs[0])], stream=s1)
            dec.decode_batch_items(d_data, d_items, out_d, *rd, stream=s2)
            assert n1.value == 0                                 # (still pending)
            dec.wait()
            assert n1.value == len(refs[0])
            torch.cuda.synchronize()
            dec.close()                                          # (while the streams its event was recorded on exist)
        for (out_len, status), o in ((ra, out_a), (rb, out_b), (rd, out_d)):
            assert not status.cpu().numpy().any()
            _check_exact(o, items, refs[1:], out_len.cpu().numpy())
        assert not st_c.any()
        _check_exact(out_c, items, refs[1:], len_c)
        assert np.array_equal(one[: len(refs[0])].cpu().numpy(), refs[0]) and _clean(one[len(refs[0]):])
    finally:
        dec.close()


def test_producer(hh):
    """Encoder.encode_blocks(..., items_out=t) leaves on the device the items
    it returns, and decode_batch_items(out, t, dst) gives the symbols back:
    block sizes on both sides of a thread's 16 symbols and of the pieces'
    4096 (tests/test_gpu_encode_blocks.py::test_breakpoints), each with a
    short last block; compress_blocks on one text."""
    import torch
    rng = np.random.default_rng(12289)
    iz, io, sy, syms = _random_tree(rng, 40)
    text = rng.choice(syms, size=3 * 12289 + 1, p=rng.dirichlet(np.full(40, 0.5))).astype(np.uint8)
    d_text = torch.from_numpy(text).cuda()
    tree = hh.Tree(iz, io, sy)
    enc = hh.Encoder(0)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        for Bs in (1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289):
            n = 3 * Bs + 1
            nb = 4
            cap = hh.encode_blocks_bound(tree, n, Bs)
            out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            t = torch.full((nb, 4), -1, dtype=torch.int64, device="cuda")
            items, total = enc.encode_blocks(tree, d_text[:n], Bs, out[:cap], items_out=t)
            want, witems = tree.encode_blocks(text[:n], Bs)
            assert np.array_equal(items, witems) and total == want.size - hh.PAYLOAD_PAD
            assert np.array_equal(t.cpu().numpy().view(np.uint64), items), Bs
            assert np.array_equal(out[:total].cpu().numpy(), want[:total]) and _clean(out[total:])
            dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
            out_len, status = dec.decode_batch_items(out[: total + hh.PAYLOAD_PAD], t, dst)
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any() and np.array_equal(out_len.cpu().numpy(), items[:, 3].astype(np.int64))
            assert torch.equal(dst[:n], d_text[:n]) and _clean(dst[n:]), Bs
        Bs = 64
        text = strain_text(Bs)
        n, nb = text.size, -(-text.size // Bs)
        d_text = torch.from_numpy(text).cuda()
        cap = hh.compress_blocks_bound(n, Bs)
        out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        t = torch.full((nb, 4), -1, dtype=torch.int64, device="cuda")
        ctree, items, total = enc.compress_blocks(d_text, Bs, out[:cap], items_out=t)
        want, witems = ctree.encode_blocks(text, Bs)
        assert np.array_equal(items, witems) and np.array_equal(t.cpu().numpy().view(np.uint64), items)
        assert np.array_equal(out[:total].cpu().numpy(), want[:total])
        dec.set_tree(ctree)
        dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status, summ = dec.decode_batch_items(out[: total + hh.PAYLOAD_PAD], t, dst, summary=True)
        torch.cuda.synchronize()
        assert dec.batch_summary(summ) == {"total_len": n, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        assert torch.equal(dst[:n], d_text) and _clean(dst[n:])
    finally:
        enc.close()
        dec.close()


def test_host_checked_arguments(hh):
    """What the host can see is refused before anything is enqueued, the
    output untouched: no tree, d_data off a 4-byte boundary, null pointers
    (HH_ERR_ARG); a tree past the state machine, the 300-leaf tree of
    test_gpu_batch.py::test_exact_without_resynchronisation
    (HH_ERR_UNSUPPORTED).  An empty batch is HH_OK and leaves the empty
    summary."""
    import torch
    dec = _decoder(hh, "kjv")
    bare = hh.Decoder(0)
    try:
        data = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        out = torch.full((1024,), 0xAB, dtype=torch.uint8, device="cuda")
        items = _dev_items(np.array([[0, 256, 0, 512]], np.uint64))
        out_len = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        with pytest.raises(hh.HipHuffError) as e:
            bare.decode_batch_items(data, items, out, out_len, status)
        assert e.value.status == ERR_ARG
        with pytest.raises(hh.HipHuffError) as e:
            dec.decode_batch_items(data[1:], items, out, out_len, status)
        assert e.value.status == ERR_ARG
        L = hh.lib()
        st = torch.cuda.current_stream().cuda_stream
        args = [data.data_ptr(), items.data_ptr(), out.data_ptr(), out_len.data_ptr(), status.data_ptr()]
        for k in range(5):
            a = list(args)
            a[k] = None
            rc = L.hh_decode_batch_device_items(dec._h, a[0], 4096, a[1], 1, a[2], 1024, a[3], a[4], None, st)
            assert rc == ERR_ARG, k
        assert L.hh_decode_batch_device_items(None, args[0], 4096, args[1], 1, args[2], 1024, args[3], args[4], None,
                                              st) == ERR_ARG
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
        with pytest.raises(hh.HipHuffError) as e:
            dec.decode_batch_items(data, items, out, out_len, status)
        assert e.value.status == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _clean(out) and out_len.item() == 77 and status.item() == 77
        for d in (dec, bare):
            n, s, summ = d.decode_batch_items(data, _dev_items(np.zeros((0, 4), np.uint64)), out, summary=True)
            torch.cuda.synchronize()
            assert n.numel() == 0 and s.numel() == 0
            assert d.batch_summary(summ) == {"total_len": 0, "n_failed": 0, "first_failed": NONE, "first_status": 0}
        assert _clean(out)
    finally:
        dec.close()
        bare.close()
