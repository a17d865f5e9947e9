"""The ragged blocked encode on the GPU (hh_encoder_encode_ragged,
hh_compress_ragged_device; csrc/hh_encr.hip) against the host reference
(Tree.encode_ragged, checked on its own by tests/test_encode_ragged.py): the
shapes the emulator runs there -- record edges on both sides of the threads'
16 and the chunks' 4096 symbols, runs of empty records, record counts around
a scan tile and beyond 2^20 -- uniform cuts against the blocked encode, long
codes, the round trip through Decoder.decode_batch_items with the device's
item list, errors, compress.  Every output is filled with 0xAB first: nothing
at or beyond total_bytes is written."""
import ctypes as C

import numpy as np
import pytest

import edge_cases as E
from test_encode_blocks import strain_text
from test_encode_ragged import NTEXT, from_lengths, model_items, random_cuts, shapes, uniform
from test_encode_ragged import cat64, r40  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module")
def enc(hh):
    e = hh.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def d40(r40):  # noqa: F811
    import torch
    return torch.from_numpy(r40[1]).cuda()


def _device_ragged(hh, enc, tree, d_syms, offs, want, witems, host_items=True, upload=False):
    """Encoder.encode_ragged of d_syms into 0xAB with exactly the host's
    total as capacity: bytes, items, items_out and total the host's, the rest
    untouched."""
    import torch
    total = want.size - hh.PAYLOAD_PAD
    nrec = offs.size - 1
    buf = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    t = torch.full((nrec, 4), -1, dtype=torch.int64, device="cuda")
    d_offs = offs if upload else torch.from_numpy(offs.view(np.int64)).cuda()
    items, got = enc.encode_ragged(tree, d_syms, d_offs, buf[:total], items_out=t, host_items=host_items)
    torch.cuda.synchronize()
    dev = buf.cpu().numpy()
    key = (d_syms.numel(), nrec)
    assert got == total, key
    assert (items is None) if not host_items else np.array_equal(items, witems), key
    assert np.array_equal(t.cpu().numpy().view(np.uint64), witems), key
    assert np.array_equal(dev[:total], want[:total]), (key, int(np.argmax(dev[:total] != want[:total])))
    assert (dev[total:] == 0xAB).all(), key
    return dev[:total]


def test_shapes(hh, enc, r40, d40):  # noqa: F811
    """tests/test_encode_ragged.py's shapes on one encoder, by growing then by
    shrinking record count (the workspace grows once and is kept); once with
    the offsets uploaded from a host array, once without host items."""
    c, text = r40
    S = shapes()
    refs = {k: c.tree.encode_ragged(text, S[k]) for k in S}
    order = sorted(S, key=lambda k: S[k].size)
    for i, k in enumerate(order + order[::-1]):
        _device_ragged(hh, enc, c.tree, d40, S[k], *refs[k], host_items=i != 3, upload=i == 5)


def test_short_texts(hh, enc, r40, d40):  # noqa: F811
    """Texts of 1 .. 4097 symbols (one thread, one chunk, a chunk and a
    symbol) in one record, in one-symbol records and with empties around."""
    c, text = r40
    for n in (1, 15, 16, 17, 4095, 4096, 4097):
        for offs in (np.array([0, n], np.uint64), uniform(n, 1), np.array([0, 0, n, n, n], np.uint64)):
            want, witems = c.tree.encode_ragged(text[:n], offs)
            _device_ragged(hh, enc, c.tree, d40[:n], offs, want, witems)


def test_unaligned_symbols(hh, enc, r40, d40):  # noqa: F811
    """d_syms a slice that starts at byte 1 of a 16-byte aligned tensor
    (enc_load16's byte loads): the aligned tensor's bytes."""
    import torch
    c, text = r40
    n = 3 * 4097 + 1
    offs = random_cuts(np.random.default_rng(21), n, 700)
    want, witems = c.tree.encode_ragged(text[:n], offs)
    base = _device_ragged(hh, enc, c.tree, d40[:n], offs, want, witems)
    buf = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d_syms = buf[1: 1 + n]
    d_syms.copy_(d40[:n])
    got = _device_ragged(hh, enc, c.tree, d_syms, offs, want, witems)
    assert np.array_equal(got, base)


def test_million_records(hh, enc, r40):  # noqa: F811
    """nrec = 1024 * 1024 + 1025 one-symbol and empty records: the record
    scan's top takes its second step."""
    import torch
    c, text = r40
    nrec = 1024 * 1024 + 1025
    text = np.tile(text, 9)[:300001]
    rng = np.random.default_rng(9)
    full = np.zeros(nrec, np.int64)
    full[rng.choice(nrec, size=text.size, replace=False)] = 1
    offs = np.concatenate([[0], np.cumsum(full)]).astype(np.uint64)
    want, witems = c.tree.encode_ragged(text, offs)
    assert np.array_equal(witems, model_items(c.lens, text, offs)[0])
    _device_ragged(hh, enc, c.tree, torch.from_numpy(text).cuda(), offs, want, witems)


@pytest.mark.parametrize("B", [1, 17, 4096, 4097])
def test_uniform_cuts_are_the_blocks(hh, enc, r40, d40, B):  # noqa: F811
    """offs[r] = min(n, r * B): Encoder.encode_blocks' bytes, items and total,
    bit for bit."""
    import torch
    c, text = r40
    n = min(NTEXT, 3 * B + 1 if B > 17 else 9001)
    offs = uniform(n, B)
    cap = hh.encode_blocks_bound(c.tree, n, B)
    a = torch.full((cap + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    b = torch.full((cap + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    bitems, btotal = enc.encode_blocks(c.tree, d40[:n], B, a[:cap])
    ritems, rtotal = enc.encode_ragged(c.tree, d40[:n], offs, b[:cap])
    torch.cuda.synchronize()
    assert rtotal == btotal and np.array_equal(ritems, bitems)
    assert torch.equal(a, b)


def test_long_codes(hh, enc, cat64):  # noqa: F811
    """Codes of 1..64 bits at every bit offset (the image's third word), cut
    at random offsets; 4096 one-symbol records in a chunk, the image's worst
    size; 64-bit codes only."""
    import torch
    c, text = cat64
    d_text = torch.from_numpy(text).cuda()
    rng = np.random.default_rng(64)
    n = text.size
    for offs in (random_cuts(rng, n, 50), random_cuts(rng, n, 3000, 0.4), uniform(n, 1)):
        want, witems = c.tree.encode_ragged(text, offs)
        _device_ragged(hh, enc, c.tree, d_text, offs, want, witems)
    n = 2 * 4096 + 5
    for sym, offs in ((32, uniform(n, 1)), (63, uniform(n, 1)), (63, from_lengths([3, 4096 * 2 - 1], n))):
        t = np.full(n, sym, np.uint8)
        want, witems = c.tree.encode_ragged(t, offs)
        _device_ragged(hh, enc, c.tree, torch.from_numpy(t).cuda(), offs, want, witems)


@pytest.mark.parametrize("name", ["kjv", "caterpillar40"])
def test_round_trip(hh, enc, name):
    """encode_ragged with items_out and no host items, then
    decode_batch_items with that tensor as it is: the text in place; every
    third row with new out_offs: those records, packed."""
    import torch
    c = E.code(name)
    n = 1 << 20
    rng = np.random.default_rng(E.CODE_NAMES.index(name) + 500)
    if c.probs is not None:
        syms, p = c.probs
        text = rng.choice(syms, size=n, p=p).astype(np.uint8)
    else:
        leaves = np.array(sorted(E._lengths(c.izero, c.ione, c.sym)), np.uint8)
        text = rng.choice(leaves, size=n).astype(np.uint8)
    lens = rng.integers(0, 128, size=2 * n // 64)
    lens = lens[np.cumsum(lens) <= n]
    offs = from_lengths(lens, n)
    nrec = offs.size - 1
    d_text = torch.from_numpy(text).cuda()
    tree = c.tree()
    cap = hh.encode_ragged_bound(tree, n, nrec)
    out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    t = torch.empty((nrec, 4), dtype=torch.int64, device="cuda")
    items, total = enc.encode_ragged(tree, d_text, offs, out[:cap], items_out=t, host_items=False)
    assert items is None and 0 < total <= cap
    assert int(out[total:].ne(0xAB).sum()) == 0
    dec = hh.Decoder(0, flags=c.flags)
    try:
        dec.set_tree(tree)
        dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status = dec.decode_batch_items(out[: total + hh.PAYLOAD_PAD], t, dst)
        torch.cuda.synchronize()
        assert int(status.ne(0).sum()) == 0
        assert torch.equal(out_len.cpu(), torch.from_numpy(np.diff(offs.astype(np.int64))))
        assert torch.equal(dst[:n], d_text) and int(dst[n:].ne(0xAB).sum()) == 0
        sel = t[::3].clone()
        k = sel[:, 3]
        sel[:, 2] = torch.cumsum(k, 0) - k
        m = int(k.sum())
        dst = torch.full((m + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status = dec.decode_batch_items(out[: total + hh.PAYLOAD_PAD], sel, dst)
        torch.cuda.synchronize()
        assert int(status.ne(0).sum()) == 0 and torch.equal(out_len, k)
        o = offs.astype(np.int64)
        keep = np.zeros(n, bool)
        for a, b in zip(o[:-1][::3], o[1:][::3]):
            keep[a:b] = True
        assert np.array_equal(dst[:m].cpu().numpy(), text[keep]) and int(dst[m:].ne(0xAB).sum()) == 0
    finally:
        dec.close()


def test_capacity_and_errors(hh, enc, r40, d40):  # noqa: F811
    import torch
    c, text = r40
    n = 9000
    offs = random_cuts(np.random.default_rng(2), n, 1500, 0.1)
    nrec = offs.size - 1
    want, witems = c.tree.encode_ragged(text[:n], offs)
    total = want.size - hh.PAYLOAD_PAD
    _device_ragged(hh, enc, c.tree, d40[:n], offs, want, witems)          # cap == total_bytes
    out = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    t = torch.full((nrec, 4), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(hh.HipHuffError) as e:                            # one word short
        enc.encode_ragged(c.tree, d40[:n], offs, out[: total - 4], items_out=t)
    assert e.value.status == -5 and e.value.total_bytes == total and np.array_equal(e.value.items, witems)
    assert np.array_equal(t.cpu().numpy().view(np.uint64), witems)
    assert int(out.ne(0xAB).sum()) == 0                                  # (found before a byte is written)
    # each offs rule; the decreasing pair in the second scan tile
    for what in ("first", "last", "pair_tile2"):
        bad = offs.copy()
        if what == "first":
            bad[0] = 1
        elif what == "last":
            bad[-1] = n - 1
        else:
            bad[1100], bad[1101] = bad[1101] + 1, bad[1100]
        d_bad = torch.from_numpy(bad.view(np.int64)).cuda()
        tot = C.c_uint64(77)
        rc = hh.lib().hh_encoder_encode_ragged(enc._h, C.byref(c.tree._c), d40.data_ptr(), n, d_bad.data_ptr(), nrec,
                                               out.data_ptr(), out.numel(), None, None, C.byref(tot),
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and tot.value == 0, what
        with pytest.raises(hh.HipHuffError) as e:
            enc.encode_ragged(c.tree, d40[:n], d_bad, out)
        assert e.value.status == -1, what
        assert int(out.ne(0xAB).sum()) == 0, what
    absent = d40[:n].clone()
    absent[4500] = next(v for v in range(256) if v not in c.leaves)
    with pytest.raises(hh.HipHuffError) as e:
        enc.encode_ragged(c.tree, absent, offs, out)
    assert e.value.status == -1
    with pytest.raises(hh.HipHuffError) as e:                            # out off a 4-byte boundary
        enc.encode_ragged(c.tree, d40[:n], offs, out[1:])
    assert e.value.status == -1
    assert int(out.ne(0xAB).sum()) == 0
    for k in (0, 3):                                                     # n == 0
        items, got = enc.encode_ragged(c.tree, d40[:0], np.zeros(k + 1, np.uint64), out)
        assert items.shape == (k, 4) and not items.any() and got == 0
    with pytest.raises(hh.HipHuffError) as e:                            # n == 0 and an offset that is not
        enc.encode_ragged(c.tree, d40[:0], np.array([0, 1], np.uint64), out)
    assert e.value.status == -1
    assert int(out.ne(0xAB).sum()) == 0


def test_compress_ragged(hh, enc):
    """One histogram, one tree, the records: the tree of the text's counts,
    the host reference's bytes with that tree, within compress_ragged_bound,
    and decode_batch gives the text back."""
    import torch
    text = strain_text(64)
    n = text.size
    offs = np.concatenate([random_cuts(np.random.default_rng(5), n - 64, 300), [n]]).astype(np.uint64)
    nrec = offs.size - 1
    d_text = torch.from_numpy(text).cuda()
    cap = hh.compress_ragged_bound(n, nrec)
    out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    tree, items, total = enc.compress_ragged(d_text, offs, out[:cap])
    torch.cuda.synchronize()
    want_tree = hh.Tree.from_counts(np.bincount(text, minlength=256))
    assert all(np.array_equal(a, b) for a, b in ((tree.izero, want_tree.izero), (tree.ione, want_tree.ione),
                                                 (tree.sym, want_tree.sym)))
    want, witems = tree.encode_ragged(text, offs)
    assert total == want.size - hh.PAYLOAD_PAD <= cap and np.array_equal(items, witems)
    assert int(items[-1, 1]) > 8 * 64
    dev = out.cpu().numpy()
    assert np.array_equal(dev[:total], want[:total]) and (dev[total:] == 0xAB).all()
    with pytest.raises(hh.HipHuffError) as e:                            # one word short: the size to retry with
        enc.compress_ragged(d_text, offs, out[: total - 4])
    assert e.value.status == -5 and e.value.total_bytes == total and np.array_equal(e.value.items, witems)
    assert np.array_equal(e.value.tree.izero, want_tree.izero)
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_len, status = dec.decode_batch(out[: total + hh.PAYLOAD_PAD], items, dst)
        torch.cuda.synchronize()
        assert not status.any() and np.array_equal(out_len, items[:, 3])
        assert torch.equal(dst[:n], d_text) and int(dst[n:].ne(0xAB).sum()) == 0
    finally:
        dec.close()
