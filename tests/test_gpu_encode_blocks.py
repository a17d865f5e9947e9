"""The blocked encode on the GPU (hh_encoder_encode_blocks,
hh_compress_blocks_device; csrc/hh_encb.hip) against the host reference
(Tree.encode_blocks, checked on its own by tests/test_encode_blocks.py):
bytes, items and total at block sizes on both sides of the 16-symbol threads
and the 4096-symbol pieces, long codes, symbols off 16-byte alignment, the
round trip through Decoder.decode_batch with the items as returned, capacity
and errors, compress.  Every output is filled with 0xAB first: nothing at or
beyond total_bytes is written."""
import numpy as np
import pytest

import edge_cases as E
from test_encode_blocks import strain_text
from test_gpu_encode import _random_tree

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
def random40(hh):
    """(tree, leaves, text of 3 * 12289 + 1 i.i.d. symbols, its device copy):
    shared, never written."""
    import torch
    rng = np.random.default_rng(12289)
    iz, io, sy, syms = _random_tree(rng, 40)
    p = rng.dirichlet(np.full(40, 0.5))
    text = rng.choice(syms, size=3 * 12289 + 1, p=p).astype(np.uint8)
    return hh.Tree(iz, io, sy), set(int(v) for v in syms), text, torch.from_numpy(text).cuda()


def _device_blocks(hh, enc, tree, d_syms, B, want, witems):
    """Encoder.encode_blocks of d_syms into 0xAB with exactly the host's
    total as capacity: bytes, items and total the host's, the rest untouched."""
    import torch
    total = want.size - hh.PAYLOAD_PAD
    buf = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    items, got = enc.encode_blocks(tree, d_syms, B, buf[:total])
    torch.cuda.synchronize()
    dev = buf.cpu().numpy()
    key = (d_syms.numel(), B)
    assert got == total and np.array_equal(items, witems), key
    assert np.array_equal(dev[:total], want[:total]), (key, int(np.argmax(dev[:total] != want[:total])))
    assert (dev[total:] == 0xAB).all(), key
    return dev[:total]


def test_breakpoints(hh, enc, random40):
    """Block sizes on both sides of a thread's 16 symbols and of the pieces'
    4096 (one, two and four pieces per block), texts on both sides of one and
    of three blocks, 5000 one-symbol blocks; on one encoder by growing, then by
    shrinking size."""
    tree, _, text, d_text = random40
    cases = set()
    for B in (1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289):
        cases |= {(n, B) for n in (1, B - 1, B, B + 1, 3 * B, 3 * B + 1) if n > 0}
    cases.add((5000, 1))
    order = sorted(cases, key=lambda c: (-(-c[0] // c[1]) * -(-c[1] // 4096), c))
    refs = {(n, B): tree.encode_blocks(text[:n], B) for n, B in order}
    for n, B in order + order[::-1]:
        want, witems = refs[(n, B)]
        assert witems.shape[0] == -(-n // B)
        _device_blocks(hh, enc, tree, d_text[:n], B, want, witems)


def test_long_codes(hh, enc):
    """Codes of 1..64 bits at every bit offset (the image's third word), the
    blocks starting anywhere in the text."""
    import torch
    iz, io, sy, text = E.every_offset_text(64)
    tree = hh.Tree(iz, io, sy)
    d_text = torch.from_numpy(text).cuda()
    for B in (7, 100, 4096, 4099):
        want, witems = tree.encode_blocks(text, B)
        _device_blocks(hh, enc, tree, d_text, B, want, witems)


def test_unaligned_symbols(hh, enc, random40):
    """Symbols at tensor offsets 1 and 15 and odd block sizes (blocks at odd
    addresses: enc_load16's byte loads): the aligned tensor's bytes."""
    import torch
    tree, _, text, d_text = random40
    n = 3 * 4097 + 1
    buf = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for B in (15, 17, 4097):
        want, witems = tree.encode_blocks(text[:n], B)
        base = _device_blocks(hh, enc, tree, d_text[:n], B, want, witems)
        for off in (1, 15):
            d_syms = buf[off: off + n]
            d_syms.copy_(d_text[:n])
            assert d_syms.data_ptr() % 16 == off
            got = _device_blocks(hh, enc, tree, d_syms, B, want, witems)
            assert np.array_equal(got, base), (B, off)


@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_round_trip(hh, enc, name):
    """encode_blocks, then decode_batch with the items as returned: 16 blocks
    of 65536 symbols and a last one of 1; 300 blocks of 4096 and one of 5."""
    import torch
    c = E.code(name)
    nmax = max(65536 * 16 + 1, 4096 * 300 + 5)
    rng = np.random.default_rng(E.CODE_NAMES.index(name) + 300)
    if c.probs is not None:
        syms, p = c.probs
        text = rng.choice(syms, size=nmax, p=p).astype(np.uint8)
    else:
        leaves = np.array(sorted(E._lengths(c.izero, c.ione, c.sym)), np.uint8)
        text = rng.choice(leaves, size=nmax).astype(np.uint8)
    d_text = torch.from_numpy(text).cuda()
    tree = c.tree()
    dec = hh.Decoder(0, flags=c.flags)
    try:
        dec.set_tree(tree)
        for B, n in ((65536, 65536 * 16 + 1), (4096, 4096 * 300 + 5)):
            cap = hh.encode_blocks_bound(tree, n, B)
            out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
            items, total = enc.encode_blocks(tree, d_text[:n], B, out[:cap])
            nb = -(-n // B)
            lens = np.minimum(B, n - np.arange(nb) * B)
            assert items.shape == (nb, 4) and total <= cap
            assert np.array_equal(items[:, 2], np.arange(nb) * B) and np.array_equal(items[:, 3], lens)
            assert int(out[total:].ne(0xAB).sum()) == 0
            dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
            out_len, status = dec.decode_batch(out[: total + hh.PAYLOAD_PAD], items, dst)
            torch.cuda.synchronize()
            assert not status.any() and np.array_equal(out_len, lens), (name, B)
            assert torch.equal(dst[:n], d_text[:n]), (name, B)
            assert int(dst[n:].ne(0xAB).sum()) == 0, (name, B)
    finally:
        dec.close()


def test_capacity_and_errors(hh, enc, random40):
    import torch
    tree, leaves, text, d_text = random40
    n, B = 3 * 4097 + 1, 4097
    want, witems = tree.encode_blocks(text[:n], B)
    _device_blocks(hh, enc, tree, d_text[:n], B, want, witems)          # cap == total_bytes
    total = want.size - hh.PAYLOAD_PAD
    out = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(hh.HipHuffError) as e:                            # one word short
        enc.encode_blocks(tree, d_text[:n], B, out[: total - 4])
    assert e.value.status == -5 and e.value.total_bytes == total and np.array_equal(e.value.items, witems)
    assert int(out.ne(0xAB).sum()) == 0                                  # (found before a byte is written)
    bad = d_text[:n].clone()
    bad[B + 5] = next(v for v in range(256) if v not in leaves)          # an absent symbol in a middle block
    with pytest.raises(hh.HipHuffError) as e:
        enc.encode_blocks(tree, bad, B, out)
    assert e.value.status == -1
    with pytest.raises(hh.HipHuffError) as e:                            # block_syms == 0
        enc.encode_blocks(tree, d_text[:n], 0, out)
    assert e.value.status == -1
    with pytest.raises(hh.HipHuffError) as e:                            # out off a 4-byte boundary
        enc.encode_blocks(tree, d_text[:n], B, out[1:])
    assert e.value.status == -1
    assert int(out.ne(0xAB).sum()) == 0
    items, got = enc.encode_blocks(tree, d_text[:0], B, out)             # n == 0
    assert items.shape == (0, 4) and got == 0 and int(out.ne(0xAB).sum()) == 0


@pytest.mark.parametrize("case", ["strain", "one_symbol"])
def test_compress_blocks(hh, enc, case):
    """One histogram, one tree, the blocks: the tree of the text's counts, the
    host reference's bytes with that tree, within compress_blocks_bound, and
    decode_batch gives the text back."""
    import torch
    B = 64
    text = strain_text(B) if case == "strain" else np.full(4097, 255, np.uint8)
    n = text.size
    d_text = torch.from_numpy(text).cuda()
    cap = hh.compress_blocks_bound(n, B)
    out = torch.full((cap + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    tree, items, total = enc.compress_blocks(d_text, B, out[:cap])
    torch.cuda.synchronize()
    want_tree = hh.Tree.from_counts(np.bincount(text, minlength=256))
    assert all(np.array_equal(a, b) for a, b in ((tree.izero, want_tree.izero), (tree.ione, want_tree.ione),
                                                 (tree.sym, want_tree.sym)))
    want, witems = tree.encode_blocks(text, B)
    assert total == want.size - hh.PAYLOAD_PAD <= cap and np.array_equal(items, witems)
    if case == "strain":
        assert int(items[-1, 1]) > 8 * B
    dev = out.cpu().numpy()
    assert np.array_equal(dev[:total], want[:total]) and (dev[total:] == 0xAB).all()
    with pytest.raises(hh.HipHuffError) as e:                            # one word short: the size to retry with
        enc.compress_blocks(d_text, B, out[: total - 4])
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
