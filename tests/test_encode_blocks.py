"""The blocked encode on the host (hh_encode_blocks, hh_encode_blocks_bound,
hh_compress_blocks_bound; Tree.encode_blocks): the reference the device call
(csrc/hh_encb.hip, tests/test_gpu_encode_blocks.py) is compared with.  Its
bytes, offsets and bits against the packing tools/bench_batch.py builds from
one Tree.encode per block; every block decoded back by the oracle and the
whole buffer, with the items as returned, by the batched decode's emulator;
the two bounds; the statuses.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import huffmandecoderongpus_amd as H
import edge_cases as E
from oracle import oracle as O
from test_emu_batch import bemu, run_bemu  # noqa: F401  (bemu: a fixture)
from test_gpu_encode import _random_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (1, 7, 16, 4096, 4099)


def pack_blocks(tree, text, B):
    """(data + pad, items) as tools/bench_batch.py packs them: every block
    encoded on its own by Tree.encode, at 4-byte boundaries."""
    nb = -(-len(text) // B)
    enc = [tree.encode(text[i * B: (i + 1) * B]) for i in range(nb)]
    offs, at = [], 0
    for p, b in enc:
        offs.append(at)
        at += ((b + 7) // 8 + 3) // 4 * 4
    data = np.zeros(at + H.PAYLOAD_PAD, np.uint8)
    for (p, b), o in zip(enc, offs):
        data[o: o + (b + 7) // 8] = p[: (b + 7) // 8]
    items = np.array([[o, b, i * B, min(B, len(text) - i * B)] for i, ((_, b), o) in enumerate(zip(enc, offs))],
                     np.uint64).reshape(-1, 4)
    return data, items


def sizes(B, limit):
    """(n, block_syms) pairs around blocks of B: n on both sides of one and of
    three blocks, and for every n one block of exactly n and of n + 1."""
    out = []
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 1):
        if n <= limit:
            out += [(n, B)] + ([(n, n), (n, n + 1)] if n else [])
    return sorted(set(out))


@pytest.fixture(scope="module")
def texts():
    """name -> (code, text): a 40-leaf random tree, kjv's tree, the 64-deep
    caterpillar with a code of every length at every bit offset."""
    rng = np.random.default_rng(4099)
    iz, io, sy, syms = _random_tree(rng, 40)
    r40 = SimpleNamespace(izero=iz, ione=io, sym=sy, tree=H.Tree(iz, io, sy), leaves=set(int(v) for v in syms))
    p = rng.dirichlet(np.full(40, 0.5))
    path = os.path.join(ROOT, "files", "kjv.txt.huff")
    hf = H.HuffFile.load(path)
    kjv = SimpleNamespace(izero=hf.izero, ione=hf.ione, sym=hf.sym, tree=hf.tree())
    ciz, cio, csy, ctext = E.every_offset_text(64)
    cat = SimpleNamespace(izero=ciz, ione=cio, sym=csy, tree=H.Tree(ciz, cio, csy))
    assert ctext.size > 3 * 4099 + 1
    return {"random40": (r40, rng.choice(syms, size=3 * 4099 + 1, p=p).astype(np.uint8)),
            "kjv": (kjv, O.OracleHuff.load(path).simple_decode()[20000: 20000 + 3 * 4099 + 1]),
            "every_offset": (cat, ctext)}


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("name", ["random40", "kjv", "every_offset"])
def test_host_blocks(texts, bemu, name, B):  # noqa: F811
    """Tree.encode_blocks against pack_blocks: offsets, bits, ranges and every
    byte, the zero padding and the pad included; within encode_blocks_bound;
    each block decoded back by the oracle's chain decode; the buffer with its
    items decoded by the batch emulator (rounds of 2 tiles): the text, every
    status 0, out_len the block lengths."""
    c, full = texts[name]
    for n, bs in sizes(B, full.size):
        text = full[:n]
        data, items = c.tree.encode_blocks(text, bs)
        want, witems = pack_blocks(c.tree, text, bs) if n else (np.zeros(H.PAYLOAD_PAD, np.uint8),
                                                                 np.zeros((0, 4), np.uint64))
        assert items.dtype == np.uint64 and np.array_equal(items, witems), (n, bs)
        assert data.size == want.size and np.array_equal(data, want), (n, bs)
        total = data.size - H.PAYLOAD_PAD
        assert H.encode_blocks_bound(c.tree, n, bs) >= total, (n, bs)
        if n == 0:
            continue
        lens = items[:, 3].astype(np.int64)
        assert lens.sum() == n and (items[:, 0] % 4 == 0).all()
        for o, b, oo, k in items.tolist():
            assert np.array_equal(E.oracle_prefix(c, data[o:], b), text[oo: oo + k]), (n, bs, oo)
        out = np.full(n + 256, 0xAB, np.uint8)
        rc, out_len, status, _ = run_bemu(bemu, c.izero, c.ione, c.sym, data, items, out, 2)
        assert rc == 0 and not status.any(), (n, bs, rc, status)
        assert np.array_equal(out_len.astype(np.int64), lens), (n, bs)
        assert np.array_equal(out[:n], text) and (out[n:] == 0xAB).all(), (n, bs)


def strain_text(B=64):
    """A text that strains hh_compress_blocks_bound: 255 blocks of B symbols,
    each block one frequent symbol (the symbols 0..190 in turn), then one block
    made only of the rarest symbols of the text's own tree, 191..254 once each.
    (With a single frequent symbol for all 255 blocks the rare block could not
    cost more than 7 bits per symbol: its 64 symbols would hang one bit below
    the root in a subtree of 64 leaves.  With 191 of them the rare symbols lie
    far deeper than 8 bits.)"""
    assert B == 64
    freq = np.repeat((np.arange(255) % 191).astype(np.uint8), B)
    return np.concatenate([freq, np.arange(191, 255, dtype=np.uint8)])


def test_compress_blocks_bound_under_strain():
    """One shared code: the rare block costs more than 8 bits per symbol (so
    hh_compress_bound of its own length would not hold it), and the blocked
    stream still fits hh_compress_blocks_bound = n rounded up to 4, + 4 nb."""
    B = 64
    text = strain_text(B)
    n = text.size
    tree = H.Tree.from_counts(np.bincount(text, minlength=256))
    data, items = tree.encode_blocks(text, B)
    assert items.shape == (256, 4)
    assert int(items[-1, 1]) > 8 * B, items[-1]
    total = data.size - H.PAYLOAD_PAD
    assert total == int(items[-1, 0]) + (int(items[-1, 1]) + 31) // 32 * 4
    assert H.compress_blocks_bound(n, B) == (n + 3) // 4 * 4 + 4 * 256
    assert total <= H.compress_blocks_bound(n, B)
    assert total <= H.encode_blocks_bound(tree, n, B)
    assert H.compress_blocks_bound(n, 0) == 0 and H.compress_blocks_bound(0, 7) == 0
    assert H.compress_blocks_bound(65, 64) == 68 + 8


def test_encode_blocks_errors(texts):
    c, full = texts["random40"]
    text = full[:1000].copy()
    with pytest.raises(H.HipHuffError) as e:                 # block_syms == 0
        c.tree.encode_blocks(text, 0)
    assert e.value.status == -1
    assert H.lib().hh_encode_blocks_bound(c.tree._c, 1000, 0) == 0
    data, items = c.tree.encode_blocks(text, 100)
    total = data.size - H.PAYLOAD_PAD
    with pytest.raises(H.HipHuffError) as e:                 # one byte short: the size to retry with
        c.tree.encode_blocks(text, 100, cap=total - 1)
    assert e.value.status == -5 and e.value.total_bytes == total and np.array_equal(e.value.items, items)
    again, items2 = c.tree.encode_blocks(text, 100, cap=total)    # exactly enough
    assert np.array_equal(again, data) and np.array_equal(items2, items)
    absent = next(v for v in range(256) if v not in c.leaves)
    text[-1] = absent                                        # an absent symbol in the last block
    with pytest.raises(H.HipHuffError) as e:
        c.tree.encode_blocks(text, 100)
    assert e.value.status == -1
    bad = H.Tree(np.array([-1], np.int32), np.array([-1], np.int32), np.array([0], np.uint8))
    assert H.lib().hh_encode_blocks_bound(bad._c, 10, 5) == 0        # (a root leaf: no tree)
