"""The record take on the GPU (hh_decode_batch_take; csrc/hh_batch_take.hip)
through Decoder.take_records: tests/test_take.py's shapes at the geometry the
library picks (Decoder.geometry(), Decoder.take_round_tiles()), the records
encoded by Encoder.encode_ragged on the device.  The truth is the text: the
concatenation of the taken records, out_offs its prefix sums, the statuses
test_take.model's.  Every output is 0xAB first and compared whole with its
guard.  The bad ids and rows here are refused by the plan before any load."""
import ctypes as C
import functools

import numpy as np
import pytest

import shape_cases as E
from test_take import (ALL_NAMES, ERR_ARG, ERR_CAPACITY, ERR_FORMAT, GEO, GUARD, M64, PAD, TAKE_W, _alphabet,
                       disagreements, expected, layout, model, record, records_of, summary_of, true_count)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module")
def enc(hh):
    e = hh.Encoder(0)
    yield e
    e.close()


_DECS = {}


def decoder(hh, name):
    """One decoder per code for the module; its geometry is the table's."""
    if name not in _DECS:
        c = E.any_code(name)
        d = hh.Decoder(0, flags=c.flags)
        d.set_tree(c.tree())
        g = d.geometry()
        assert (g["S"], g["K"], g["G"], g["W"]) == (GEO[name][0], GEO[name][1], GEO[name][4], GEO[name][5]), (name, g)
        assert d.take_round_tiles() == TAKE_W[name], (name, d.take_round_tiles())
        _DECS[name] = d
    return _DECS[name]


@pytest.fixture(scope="module", autouse=True)
def _close_decoders():
    yield
    for d in _DECS.values():
        d.close()
    _DECS.clear()


def encode_on_device(hh, enc, name, text, offs, stream=None):
    """Encoder.encode_ragged: (data with its pad, the device item list)."""
    import torch
    tree = E.any_code(name).tree()
    nrec = len(offs) - 1
    cap = hh.encode_ragged_bound(tree, len(text), nrec)
    buf = torch.zeros(cap + PAD, dtype=torch.uint8, device="cuda")
    t = torch.full((nrec, 4), -1, dtype=torch.int64, device="cuda")
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_offs = torch.from_numpy(np.asarray(offs, np.uint64).view(np.int64)).cuda()
    _, total = enc.encode_ragged(tree, d_text, d_offs, buf[:cap], items_out=t, host_items=False, stream=stream)
    return buf[: total + PAD], t


@functools.lru_cache(maxsize=None)
def _host_case(name):
    S = GEO[name][0]
    text, offs, data, index, marks = layout(name, TAKE_W[name], S)
    return text, offs, data, index, marks, records_of(text, offs)


_DEV = {}


def case(hh, enc, name):
    """layout() at the library's geometry, encoded on the device (the items
    are the host encoder's)."""
    text, offs, data, index, marks, recs = _host_case(name)
    if name not in _DEV:
        d, t = encode_on_device(hh, enc, name, text, offs)
        assert np.array_equal(t.cpu().numpy().view(np.uint64), index), name
        _DEV[name] = (d, t)
    return _DEV[name] + (index, marks, recs)


def take(dec, data, index_t, ids, out_bytes, shift=0, stream=None, data_bytes=None):
    """One take into 0xAB: (out, out_offs, status, summary)."""
    import torch
    m = index_t.shape[0] if ids is None else len(ids)
    buf = torch.full((16 + out_bytes + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    out = buf[shift: shift + out_bytes + GUARD]
    offs = torch.full((m + 1,), 77, dtype=torch.int64, device="cuda")
    status = torch.full((m,), 77, dtype=torch.int32, device="cuda")
    summ = torch.full((6,), 77, dtype=torch.int32, device="cuda")
    ids_t = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, np.uint64).view(np.int64)).cuda()
    dec.take_records(data, index_t, ids_t, out, out_offs=offs, status=status, summary=summ, stream=stream,
                     out_bytes=out_bytes, data_bytes=data_bytes)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return (out.cpu().numpy(), offs.cpu().numpy().view(np.uint64).tolist(), status.cpu().numpy().tolist(),
            dec.batch_summary(summ))


def check(got, index, ids, data_bytes, out_bytes, recs, counts=None):
    out, offs, status, summary = got
    idx = np.asarray(index, np.uint64).tolist()
    ids_l = list(range(len(idx))) if ids is None else [int(i) for i in ids]
    w_offs, w_status, deliv = model(idx, ids_l, data_bytes, out_bytes, counts)
    assert offs == w_offs
    assert status == w_status, [(j, a, b) for j, (a, b) in enumerate(zip(status, w_status)) if a != b][:8]
    want = expected(out.size, w_offs, deliv, ids_l, recs)
    assert np.array_equal(out, want), int(np.argmax(out != want))
    assert summary == summary_of(w_offs, w_status), (summary, summary_of(w_offs, w_status))


@pytest.mark.parametrize("name", ALL_NAMES)
def test_round_edges(hh, enc, name):
    """layout()'s records -- one, two and three regions, bits of k S and k S
    +- 1 and 1, a record that ends in a round's last slot, one that starts in
    slot 0, one that starts in the last slot and is carried, a stream of 2.5
    rounds among one-region records, runs of 1500 empties at the start,
    inside and at the end -- all taken in order."""
    dec = decoder(hh, name)
    data, t, index, marks, recs = case(hh, enc, name)
    total = int(index[:, 3].sum())
    check(take(dec, data, t, None, total), index, None, data.numel(), total, recs)


@pytest.mark.parametrize("name", ["kjv", "byte256", "fixed1", "lattice5"])
def test_ids(hh, enc, name):
    """A random permutation, a subset, every id twice, one record 1000 times,
    ids equal to nrec and 2^64 - 1 among good ones."""
    dec = decoder(hh, name)
    data, t, index, marks, recs = case(hh, enc, name)
    nrec = index.shape[0]
    rng = np.random.default_rng(5)
    bad = np.arange(1490, 1600, dtype=np.uint64)
    bad[[3, 50, 51, 109]] = [nrec, M64, nrec + 1, M64 - 1]
    for ids in (rng.permutation(nrec).astype(np.uint64),
                np.sort(rng.choice(nrec, nrec // 3, replace=False)).astype(np.uint64),
                np.repeat(np.arange(nrec, dtype=np.uint64), 2), np.full(1000, marks["carry"], np.uint64), bad):
        total = int(sum(index[int(i), 3] for i in ids if i < nrec))
        check(take(dec, data, t, ids, total), index, ids, data.numel(), total, recs)


def test_bad_rows_and_empties(hh, enc):
    """data_off odd, a payload past data_bytes, data_off near 2^64:
    HH_ERR_ARG, length 0, the others exact.  All records empty.  m == 0: the
    empty summary, nothing else written."""
    import torch
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    idx = index.copy()
    a, b, c = 1510, 1511, marks["carry"]
    idx[a, 0] += 2
    idx[b, 0] = data.numel() - PAD
    idx[c, 0] = M64 - 3
    total = int(idx[:, 3].sum()) - int(idx[[a, b, c], 3].sum())
    got = take(dec, data, torch.from_numpy(idx.view(np.int64)).cuda(), None, total)
    check(got, idx, None, data.numel(), total, recs)
    assert got[2][a] == got[2][b] == got[2][c] == ERR_ARG
    zero = np.zeros((3000, 4), np.uint64)
    got = take(dec, data, torch.from_numpy(zero.view(np.int64)).cuda(), None, 16)
    check(got, zero, None, data.numel(), 16, [np.zeros(0, np.uint8)] * 3000)
    out, offs, status, summary = take(dec, data, t, np.zeros(0, np.uint64), 16)
    assert (out == 0xAB).all() and offs == [77]
    assert summary == {"total_len": 0, "n_failed": 0, "first_failed": 0xffffffff, "first_status": 0}


@pytest.mark.parametrize("name", ["kjv", "complete7"])
def test_index_and_data_disagree(hh, enc, name):
    """test_take.disagreements on the GPU: HH_ERR_FORMAT on that record
    alone, min(c, len) bytes delivered, the rest of its range 0xAB, every
    other record exact -- a record among good ones in its round, and the long
    stream."""
    import torch
    dec = decoder(hh, name)
    data, t, index, marks, recs = case(hh, enc, name)
    hdata = data.cpu().numpy()
    S = GEO[name][0]
    for what, r, field, value in disagreements(name, index, marks, recs, S, 64 * TAKE_W[name]):
        idx = index.copy()
        idx[r, field] = value
        dec_r = true_count(name, hdata, idx[r])
        counts = idx[:, 3].tolist()
        counts[r] = len(dec_r)
        rr = list(recs)
        rr[r] = dec_r
        total = int(idx[:, 3].sum())
        got = take(dec, data, torch.from_numpy(idx.view(np.int64)).cuda(), None, total)
        check(got, idx, None, data.numel(), total, rr, counts)
        assert got[2][r] == ERR_FORMAT and got[3]["n_failed"] == 1, what


def test_capacity(hh, enc):
    """out_bytes the total, one byte less, half a record, 0."""
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    total = int(index[:, 3].sum())
    k = marks["carry"]
    for ob in (total, total - 1, int(index[:k, 3].sum()) + int(index[k, 3]) // 2, 0):
        got = take(dec, data, t, None, ob)
        check(got, index, None, data.numel(), ob, recs)
        assert got[1][-1] == total and (ob == total or ERR_CAPACITY in got[2])


@pytest.mark.parametrize("shift", [1, 3, 15])
def test_alignment(hh, enc, shift):
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    total = int(index[:, 3].sum())
    check(take(dec, data, t, None, total, shift=shift), index, None, data.numel(), total, recs)


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_scan_tiles(hh, enc, m):
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    ids = np.arange(1400, 1400 + m, dtype=np.uint64)
    total = int(index[1400: 1400 + m, 3].sum())
    check(take(dec, data, t, ids, total), index, ids, data.numel(), total, recs)


def test_million_records(hh, enc):
    """2^20 + 1025 one-symbol and empty records over 300001 symbols: the
    scans' top takes its second step; compared as arrays."""
    import torch
    name = "kjv"
    dec = decoder(hh, name)
    nrec = 1024 * 1024 + 1025
    rng = np.random.default_rng(9)
    syms, _, p, _, _ = _alphabet(name)
    text = rng.choice(syms, size=300001, p=p).astype(np.uint8)
    full = np.zeros(nrec, np.int64)
    full[rng.choice(nrec, size=text.size, replace=False)] = 1
    offs = np.concatenate([[0], np.cumsum(full)]).astype(np.uint64)
    data, t = encode_on_device(hh, enc, name, text, offs)
    buf = torch.full((text.size + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    o, s, summ = dec.take_records(data, t, None, buf, summary=True, out_bytes=text.size)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy().view(np.uint64), offs) and not s.any().item()
    got = buf.cpu().numpy()
    assert np.array_equal(got[: text.size], text) and (got[text.size:] == 0xAB).all()
    assert dec.batch_summary(summ) == {"total_len": text.size, "n_failed": 0, "first_failed": 0xffffffff,
                                       "first_status": 0}


def test_many_workgroups(hh, enc):
    """More streams than resident workgroups times one round: 300000 records
    of 1 .. 60 symbols and a stream of many rounds in their middle, which
    straddles share edges (its workgroup finishes it, the next begins at the
    next stream).  A few MiB of text."""
    import torch
    name = "kjv"
    dec = decoder(hh, name)
    rng = np.random.default_rng(31)
    syms, _, p, _, _ = _alphabet(name)
    lens = rng.integers(1, 61, 300000)
    lens[150000] = 600000
    lens[7] = 0
    text = rng.choice(syms, size=int(lens.sum()), p=p).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data, t = encode_on_device(hh, enc, name, text, offs)
    buf = torch.full((3 + text.size + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    o, s = dec.take_records(data, t, None, buf[3:], out_bytes=text.size)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy().view(np.uint64), offs) and not s.any().item()
    got = buf.cpu().numpy()
    assert np.array_equal(got[3: 3 + text.size], text) and (got[:3] == 0xAB).all() and (got[3 + text.size:] == 0xAB).all()


def test_summaries_across_workgroups(hh, enc):
    """Failures in four different workgroups of the results kernel (256
    records each): first_failed is the lowest, n_failed the count."""
    import torch
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    nrec = index.shape[0]
    ids = np.arange(nrec, dtype=np.uint64)
    bad = [1600 + 300, 1600 + 2 * 300 + 5, 1600 + 4 * 256 + 1, nrec - 2]
    ids[bad[0]] = M64
    ids[bad[2]] = nrec
    idx = index.copy()
    idx[bad[1], 3] += 1
    idx[nrec - 2, 0] = 2
    assert len({b // 256 for b in bad}) == 4
    total = int(sum(idx[int(i), 3] for j, i in enumerate(ids) if i < nrec and j != nrec - 2))
    dec_r = list(recs)
    got = take(dec, data, torch.from_numpy(idx.view(np.int64)).cuda(), ids, total)
    check(got, idx, ids, data.numel(), total, dec_r, index[:, 3].tolist())
    assert got[3]["n_failed"] == 4 and got[3]["first_failed"] == bad[0] and got[3]["first_status"] == ERR_ARG


def test_stream_order(hh):
    """A take enqueued directly after Encoder.encode_ragged(..., items_out=t)
    on one non-default stream, nothing between them; then a second take on
    another stream (it waits for the first one's end: one workspace)."""
    import torch
    name = "kjv"
    text, offs, _, index, marks, recs = _host_case(name)
    tree = E.any_code(name).tree()
    nrec = index.shape[0]
    total = int(index[:, 3].sum())
    dec = decoder(hh, name)
    e2 = hh.Encoder(0)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        cap = hh.encode_ragged_bound(tree, len(text), nrec)
        buf = torch.zeros(cap + PAD, dtype=torch.uint8, device="cuda")
        t = torch.full((nrec, 4), -1, dtype=torch.int64, device="cuda")
        d_text = torch.zeros(len(text), dtype=torch.uint8, device="cuda")
        h_text = torch.from_numpy(text).pin_memory()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        o1 = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        o2 = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        ids2 = torch.from_numpy(np.arange(nrec - 1, -1, -1, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            d_text.copy_(h_text, non_blocking=True)          # (work queued ahead of the encode)
            e2.encode_ragged(tree, d_text, d_offs, buf[:cap], items_out=t, host_items=False, stream=s1)
            a = dec.take_records(buf, t, None, o1, summary=True, stream=s1, out_bytes=total)
        b = dec.take_records(buf, t, ids2, o2, summary=True, stream=s2, out_bytes=total)
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
    finally:
        e2.close()
    w_offs, w_status, deliv = model(index.tolist(), list(range(nrec)), buf.numel(), total)
    assert a[0].cpu().numpy().view(np.uint64).tolist() == w_offs and not a[1].any().item()
    assert np.array_equal(o1.cpu().numpy(), expected(total + GUARD, w_offs, deliv, list(range(nrec)), recs))
    rev = list(range(nrec - 1, -1, -1))
    w_offs, w_status, deliv = model(index.tolist(), rev, buf.numel(), total)
    assert b[0].cpu().numpy().view(np.uint64).tolist() == w_offs and not b[1].any().item()
    assert np.array_equal(o2.cpu().numpy(), expected(total + GUARD, w_offs, deliv, rev, recs))
    assert dec.batch_summary(a[2])["total_len"] == total == dec.batch_summary(b[2])["total_len"]


def test_the_other_entry_point(hh, enc):
    """Taking all records gives the bytes of decode_batch_items on the same
    list (whose out_off is the record's offset)."""
    import torch
    dec = decoder(hh, "byte256")
    data, t, index, marks, recs = case(hh, enc, "byte256")
    total = int(index[:, 3].sum())
    a = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    b = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    ln, s1 = dec.decode_batch_items(data, t, a, out_bytes=total)
    o, s2 = dec.take_records(data, t, None, b, out_bytes=total)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not s1.any().item() and not s2.any().item()
    assert torch.equal(o[1:] - o[:-1], ln)


def test_blocked_index(hh, enc):
    """A blocked buffer taken by block id (Encoder.encode_blocks' list)."""
    import torch
    name = "kjv"
    dec = decoder(hh, name)
    W, S = TAKE_W[name], GEO[name][0]
    text, B, _, index = E.blocked(name, W, S)
    tree = E.any_code(name).tree()
    cap = hh.encode_blocks_bound(tree, len(text), B)
    buf = torch.zeros(cap + PAD, dtype=torch.uint8, device="cuda")
    t = torch.full((index.shape[0], 4), -1, dtype=torch.int64, device="cuda")
    enc.encode_blocks(tree, torch.from_numpy(text).cuda(), B, buf[:cap], items_out=t)
    recs = [text[i: i + B] for i in range(0, len(text), B)]
    ids = np.array([4, 0, 2, 2, 1, 3], np.uint64)
    total = int(sum(len(recs[int(i)]) for i in ids))
    check(take(dec, buf, t, ids, total), index, ids, buf.numel(), total, recs)


def test_host_checks(hh, enc):
    """What the host refuses before anything is enqueued."""
    import torch
    dec = decoder(hh, "kjv")
    data, t, index, marks, recs = case(hh, enc, "kjv")
    L = hh.lib()
    nrec = index.shape[0]
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    offs = torch.full((nrec + 2,), 77, dtype=torch.int64, device="cuda")
    st = torch.full((nrec,), 77, dtype=torch.int32, device="cuda")
    ids = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = [dec._h, data.data_ptr(), data.numel(), t.data_ptr(), nrec, ids.data_ptr(), 4, out.data_ptr(), 64,
            offs.data_ptr(), st.data_ptr(), None, None]
    for k, v in ((0, None), (1, None), (1, data.data_ptr() + 2), (3, None), (7, None), (9, None),
                 (9, offs.data_ptr() + 4), (10, None)):
        a = list(good)
        a[k] = v
        assert L.hh_decode_batch_take(*a) == -1, k
    a = list(good)
    a[5], a[6] = None, 4                                     # (ids == NULL with m != nrec)
    assert L.hh_decode_batch_take(*a) == -1
    for k, v in ((6, (1 << 32) - 1), (4, (1 << 32) - 1)):
        a = list(good)
        a[k] = v
        assert L.hh_decode_batch_take(*a) == -10, k
    fresh = hh.Decoder(0)
    try:
        a = list(good)
        a[0] = fresh._h
        assert L.hh_decode_batch_take(*a) == -1              # (no tree set)
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert (out == 0xAB).all().item() and (offs == 77).all().item() and (st == 77).all().item()
