"""GPU compression (hh_histogram_device, hh_compress_device; csrc/hh_hist.hip,
csrc/hh_encode.hip): the byte histogram against np.bincount at sizes around
its 16-byte vectors and at unaligned base pointers (with a canary value
around the slice), past one sweep of its persistent grid and past 2^32
equal bytes (in stream order: tests/test_gpu_stream_order.py); the one-call compress against the Python tree
builder, the shipped headers' bit counts (an optimal code's cost is unique:
an exact check), the host encoder's bytes, the GPU decoder and the oracle;
its errors; the CLI's compress command."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xEE
# fixtures whose originals are in files/, and their headers' bits
FIXTURES = {"hello": 32, "paper1": 266692, "book2": 2946397, "news": 1971146,
            "bible.txt": 17747595, "world192.txt": 12468759}
HIST_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 1_000_003]


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
def skewed():
    """1 000 003 Dirichlet-skewed bytes without the canary value (host copy,
    device copy): shared, never written."""
    import torch
    rng = np.random.default_rng(77)
    vals = np.array([v for v in range(256) if v != CANARY], np.uint8)
    p = rng.dirichlet(np.full(vals.size, 0.5))
    data = rng.choice(vals, size=max(HIST_SIZES), p=p).astype(np.uint8)
    return data, torch.from_numpy(data).cuda()


def _text(files_dir, name):
    return np.fromfile(os.path.join(files_dir, name), np.uint8)


def _same_tree(a, b):
    return (np.array_equal(a.izero, b.izero) and np.array_equal(a.ione, b.ione)
            and np.array_equal(a.sym, b.sym))


def _tiled(text, n):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    return t.repeat(n // t.numel() + 1)[:n].contiguous()


def _tiled_counts(text, n):
    full, rest = divmod(n, len(text))
    return (np.bincount(text, minlength=256) * full + np.bincount(text[:rest], minlength=256)).astype(np.uint64)


@pytest.mark.parametrize("off", [0, 1, 7])
@pytest.mark.parametrize("n", HIST_SIZES)
def test_histogram_matches_bincount(enc, skewed, n, off):
    import torch
    data, d_data = skewed
    buf = torch.full((n + 64,), CANARY, dtype=torch.uint8, device="cuda")
    buf[off:off + n] = d_data[:n]
    sl = buf[off:off + n]
    assert n == 0 or sl.data_ptr() % 16 == off
    got = enc.histogram(sl)
    assert got.dtype == np.uint64 and got.shape == (256,)
    assert got[CANARY] == 0                               # nothing outside the slice was read
    assert np.array_equal(got, np.bincount(data[:n], minlength=256).astype(np.uint64))


def test_histogram_module_function(hh, skewed):
    data, d_data = skewed
    got = hh.histogram_device(d_data[:4097])
    assert np.array_equal(got, np.bincount(data[:4097], minlength=256).astype(np.uint64))


def test_histogram_grid_stride_wrap(enc, files_dir):
    """More than one sweep of the persistent grid, and a ragged end."""
    text = _text(files_dir, "bible.txt")
    n = (64 << 20) + 5
    got = enc.histogram(_tiled(text, n))
    assert np.array_equal(got, _tiled_counts(text, n))


def test_histogram_constant_past_2_32(enc):
    """Every byte on one counter: the u32 partial sums to the u64 total."""
    import torch
    n = 2 ** 32 + 4096
    d = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    got = enc.histogram(d)
    del d
    want = np.zeros(256, np.uint64)
    want[7] = n
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_compress_fixture(hh, enc, files_dir, name):
    import torch
    from huffmandecoderongpus_amd import synth
    text = _text(files_dir, name)
    n = len(text)
    d_syms = torch.from_numpy(text).cuda()
    out = torch.full((hh.compress_bound(n) + hh.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
    tree, bits = enc.compress(d_syms, out)
    torch.cuda.synchronize()
    # the tree: the Python builder's, node for node; the cost: the shipped header's
    assert _same_tree(tree, synth.huffman_tree(np.bincount(text, minlength=256)))
    shipped = hh.HuffFile.load(os.path.join(files_dir, name + ".huff"))
    assert shipped.bits == FIXTURES[name] and bits == shipped.bits
    # the payload: the host encoder's with that tree; nothing past the last word
    dev = out.cpu().numpy()
    host, hbits = tree.encode(text)
    nb = (bits + 7) // 8
    assert hbits == bits and np.array_equal(dev[:nb], host[:nb])
    assert (dev[(bits + 31) // 32 * 4:] == 0xAB).all()
    # decoded back by the GPU decoder (the pad zeroed, as a loaded payload's is)
    out[(bits + 31) // 32 * 4:] = 0
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        got = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
        m = dec.decode_device(out, bits, got)
        torch.cuda.synchronize()
        assert m == n and torch.equal(got[:m], d_syms)
    finally:
        dec.close()
    # and by the oracle
    hf = O.Huff(bits, 0, tree.izero, tree.ione, tree.sym, dev[:nb])
    assert np.array_equal(O.OracleHuff.from_arrays(hf).chain_decode(), text)


def test_compress_device_container(hh, files_dir, tmp_path):
    """compress_device: a HuffFile that saves, loads and decodes."""
    import torch
    text = _text(files_dir, "paper1")
    hf = hh.compress_device(torch.from_numpy(text).cuda())
    assert hf.bits == FIXTURES["paper1"] and hf.uncompressedsize == len(text)
    assert hf.data.size == (hf.bits + 7) // 8 + hh.PAYLOAD_PAD and not hf.data[len(hf.payload):].any()
    p = str(tmp_path / "p.huff")
    hf.save(p)
    assert np.array_equal(O.OracleHuff.load(p).simple_decode(), text)


def test_compress_large_round_trip(hh, enc, files_dir):
    import torch
    n = 64 << 20
    d_syms = _tiled(_text(files_dir, "bible.txt"), n)
    out = torch.zeros(hh.compress_bound(n) + hh.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
    tree, bits = enc.compress(d_syms, out)
    assert bits <= 8 * n
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        got = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
        m = dec.decode_device(out, bits, got)
        torch.cuda.synchronize()
        assert m == n and torch.equal(got[:m], d_syms)
    finally:
        dec.close()


def _small_cases():
    two = np.array([3, 9] * 700 + [9] * 501, np.uint8)
    return {"one_symbol_1": np.full(1, 65, np.uint8), "one_symbol_4097": np.full(4097, 255, np.uint8),
            "two_symbols": two, "all_256_x17": np.repeat(np.arange(256, dtype=np.uint8), 17)}


@pytest.mark.parametrize("case", ["one_symbol_1", "one_symbol_4097", "two_symbols", "all_256_x17"])
def test_compress_small_round_trip(hh, enc, case):
    import torch
    text = _small_cases()[case]
    if case == "all_256_x17":
        text = np.random.default_rng(3).permutation(text)
    n = len(text)
    d_syms = torch.from_numpy(text).cuda()
    out = torch.zeros(hh.compress_bound(n) + hh.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
    tree, bits = enc.compress(d_syms, out)
    if case.startswith("one_symbol") or case == "two_symbols":
        assert bits == n
    else:
        assert bits == 8 * n and tree.info()["minlen"] == 8
    dec = hh.Decoder(0)
    try:
        dec.set_tree(tree)
        got = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
        m = dec.decode_device(out, bits, got)
        torch.cuda.synchronize()
        if case == "all_256_x17":
            assert dec.stats()["fixed_length"] == 1
        assert m == n and torch.equal(got[:m], d_syms)
    finally:
        dec.close()


def test_compress_long_codes(hh, enc):
    """Exactly the 34-symbol Fibonacci counts (14 930 351 symbols, codes up
    to 33 bits), shuffled: the bit count and the host encoder's bytes."""
    import torch
    from huffmandecoderongpus_amd import synth
    c = [1, 1]
    while len(c) < 34:
        c.append(c[-1] + c[-2])
    counts = np.zeros(256, np.int64)
    counts[100:134] = c
    text = np.repeat(np.arange(256, dtype=np.uint8), counts)
    assert text.size == 14_930_351
    np.random.default_rng(34).shuffle(text)
    d_syms = torch.from_numpy(text).cuda()
    out = torch.zeros(hh.compress_bound(text.size) + hh.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
    tree, bits = enc.compress(d_syms, out)
    torch.cuda.synchronize()
    lens = synth.code_lengths(tree)
    assert lens.max() == 33 and bits == int((counts * lens).sum())
    host, hbits = tree.encode(text)
    nb = (bits + 7) // 8
    assert hbits == bits and np.array_equal(out[:nb].cpu().numpy(), host[:nb])


def test_compress_errors(hh, enc, files_dir):
    import torch
    from huffmandecoderongpus_amd import synth
    text = _text(files_dir, "paper1")
    d_syms = torch.from_numpy(text).cuda()
    need = (FIXTURES["paper1"] + 31) // 32 * 4
    out = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    # one word short: capacity, with the bits and the tree filled
    with pytest.raises(hh.HipHuffError) as e:
        enc.compress(d_syms, out[: need - 4])
    assert e.value.status == -5 and e.value.bits == FIXTURES["paper1"]
    assert _same_tree(e.value.tree, synth.huffman_tree(np.bincount(text, minlength=256)))
    assert not out.any().item()                          # (found before any encode kernel ran)
    tree, bits = enc.compress(d_syms, out[:need])        # exactly enough
    assert bits == FIXTURES["paper1"]
    with pytest.raises(hh.HipHuffError) as e:            # n == 0
        enc.compress(d_syms[:0], out)
    assert e.value.status == -1
    with pytest.raises(hh.HipHuffError) as e:            # misaligned out
        enc.compress(d_syms, out[1:])
    assert e.value.status == -1


def test_cli_compress(hh, files_dir, tmp_path):
    exe = os.path.join(ROOT, "build", "HuffFramework")
    src = os.path.join(files_dir, "paper1")
    p = str(tmp_path / "p.huff")
    r = subprocess.run([exe, "compress", src, p], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits 266692, uncompressedsize 53161" in r.stdout
    hf = hh.HuffFile.load(p)
    assert hf.bits == 266692 and hf.uncompressedsize == 53161
    assert np.array_equal(hh.decode_file(p), _text(files_dir, "paper1"))
