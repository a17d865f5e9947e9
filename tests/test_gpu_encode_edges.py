"""The device encoder (csrc/hh_encode.hip) where tests/test_gpu_encode.py
does not reach: codes of more than 33 bits (k_enc_pack's third image word)
and symbols at an address off 16-byte alignment (enc_load16's byte loads)."""
import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_encode import _encode_both, _random_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


def _encode_dev(hh, tree, d_syms, hbits):
    """(device bytes, device bits) of hh_encode_device on the CUDA tensor
    d_syms as it is (its own address), into a buffer of the host stream's
    words + pad filled with 0xAB: nothing is written past the last word."""
    import torch
    cap = (hbits + 31) // 32 * 4 + hh.PAYLOAD_PAD
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    dbits = hh.encode_device(tree, d_syms, out)
    torch.cuda.synchronize()
    dev = out.cpu().numpy()
    assert (dev[(dbits + 31) // 32 * 4:] == 0xAB).all()
    return dev[: (dbits + 7) // 8], dbits


def test_encode_device_long_codes(hh):
    """Codes of 1..64 bits (a 64-deep caterpillar; the ABI and the host
    encoder take codes of up to 64 bits): k_enc_pack's third image word, for a
    code that starts at bit o of a word and is longer than 64 - o bits, needs
    a code of 34 bits or more.  The text with a code of every length at every
    offset (edge_cases.every_offset_text, checked on the host by
    test_emu_edges.py::test_host_encoder_every_offset_and_length) and uniform
    random leaves at sizes around the 16-symbol threads and the 4096-symbol
    chunks: the host encoder's bytes, decoded back by the oracle and by the
    GPU decoder."""
    import torch
    import edge_cases as E
    iz, io, sy, text = E.every_offset_text(64)
    tree = hh.Tree(iz, io, sy)
    assert tree.info()["maxlen"] == 64
    rng = np.random.default_rng(64)
    texts = [text] + [rng.integers(0, 65, n).astype(np.uint8) for n in (1, 15, 16, 17, 4095, 4096, 4097, 100_003)]
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        for t in texts:
            host, hbits, dev, dbits = _encode_both(hh, tree, t)
            assert dbits == hbits, t.size
            assert np.array_equal(dev, host), (t.size, int(np.argmax(dev != host)))
            hf = O.Huff(dbits, 0, np.asarray(iz, np.int32), np.asarray(io, np.int32), np.asarray(sy, np.uint8), dev)
            back = O.OracleHuff.from_arrays(hf).chain_decode()
            assert np.array_equal(back, t), t.size
            pay = np.zeros(len(dev) + 3 & ~3, np.uint8)
            pay[: len(dev)] = dev
            d_in = torch.from_numpy(np.concatenate([pay, np.zeros(hh.PAYLOAD_PAD, np.uint8)])).cuda()
            got = torch.full((t.size + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
            n = dec.decode_device(d_in, dbits, got)
            torch.cuda.synchronize()
            st = dec.stats()
            assert n == t.size and np.array_equal(got[:n].cpu().numpy(), t), (t.size, n, st)
            assert int(got[n:].ne(0xAB).sum()) == 0, (t.size, st)
    finally:
        dec.close()


def test_encode_device_unaligned_symbols(hh):
    """Symbols at an address off 16-byte alignment (enc_load16's byte-by-byte
    loads; every other test passes a tensor's own, aligned, address): the same
    bytes as from the aligned tensor and from the host encoder, at sizes
    around the 16-symbol threads and the 4096-symbol chunks; and the same
    tree, bits and bytes through Encoder.compress."""
    import torch
    rng = np.random.default_rng(1640)
    iz, io, sy, syms = _random_tree(rng, 40)
    tree = hh.Tree(iz, io, sy)
    p = rng.dirichlet(np.full(40, 0.5))
    enc = hh.Encoder(0)
    try:
        for n in (1, 15, 16, 17, 4095, 4096, 4097, 8193):
            text = rng.choice(syms, size=n, p=p).astype(np.uint8)
            host, hbits, dev, dbits = _encode_both(hh, tree, text)
            assert dbits == hbits and np.array_equal(dev, host), n
            buf = torch.full((n + 32,), 0xAB, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            for off in (1, 3, 8, 15):
                d_syms = buf[off: off + n]
                d_syms.copy_(torch.from_numpy(text))
                assert d_syms.data_ptr() % 16 == off
                got, gbits = _encode_dev(hh, tree, d_syms, hbits)
                assert gbits == hbits, (n, off)
                assert np.array_equal(got, dev) and np.array_equal(got, host), (n, off)
            # compress: the text's own Huffman tree, from the aligned and the unaligned symbols
            cap = hh.compress_bound(n) + hh.PAYLOAD_PAD
            out0 = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
            t0, bits0 = enc.compress(torch.from_numpy(text).cuda(), out0)
            torch.cuda.synchronize()
            want, wbits = t0.encode(text)
            assert bits0 == wbits
            assert np.array_equal(out0[: (bits0 + 7) // 8].cpu().numpy(), want[: (wbits + 7) // 8]), n
            for off in (1, 15):
                d_syms = buf[off: off + n]
                d_syms.copy_(torch.from_numpy(text))
                assert d_syms.data_ptr() % 16 == off
                out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
                t1, bits1 = enc.compress(d_syms, out)
                torch.cuda.synchronize()
                assert bits1 == bits0, (n, off)
                assert all(np.array_equal(a, b) for a, b in ((t1.izero, t0.izero), (t1.ione, t0.ione), (t1.sym, t0.sym)))
                assert torch.equal(out, out0), (n, off)
    finally:
        enc.close()
