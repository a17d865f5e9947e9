"""bench.py --dump-outputs (dump_outputs): the arrays it writes for a small
output (whole) and for one past DUMP_WHOLE (both ends, the seeded sample,
the block sums), on host tensors -- no GPU."""
import os

import numpy as np
import pytest
import torch

import bench


def _symbols(n: int) -> np.ndarray:
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) >> np.uint64(13)).astype(np.uint8)


def _load(d, name):
    return np.load(os.path.join(d, name + ".npy"))


def _block_sums(sym: np.ndarray) -> np.ndarray:
    B = bench.DUMP_BLOCK
    return np.array([sym[o:o + B].sum(dtype=np.int64) for o in range(0, sym.size, B)], np.float64)


@pytest.mark.parametrize("n", [1, 1000, bench.DUMP_BLOCK, bench.DUMP_BLOCK + 7])
def test_dump_small_output_is_whole(tmp_path, n):
    sym = _symbols(n)
    buf = torch.from_numpy(np.concatenate([sym, np.full(64, 0xAA, np.uint8)]))   # (slack past n never read)
    bench.dump_outputs(str(tmp_path), buf, n)
    assert sorted(os.listdir(tmp_path)) == ["decoded_block_sums.npy", "decoded_length.npy", "decoded_symbols.npy"]
    ln, got, sums = (_load(tmp_path, k) for k in ("decoded_length", "decoded_symbols", "decoded_block_sums"))
    assert ln.dtype == np.float64 and ln.tolist() == [n]
    assert got.dtype == np.float32 and np.array_equal(got, sym.astype(np.float32))
    assert sums.dtype == np.float64 and np.array_equal(sums, _block_sums(sym))


def test_dump_large_output_is_sampled(tmp_path):
    n = bench.DUMP_WHOLE + 12345
    sym = _symbols(n)
    buf = torch.from_numpy(sym)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), buf, n, "_rank1")
    bench.dump_outputs(str(b), buf, n, "_rank1")
    got = _load(a, "decoded_symbols_rank1")
    E, S = bench.DUMP_EDGE, bench.DUMP_SAMPLE
    assert got.dtype == np.float32 and got.size == 2 * E + S
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(E, n - E, S))
    assert np.array_equal(got[:E], sym[:E]) and np.array_equal(got[E + S:], sym[n - E:])
    assert np.array_equal(got[E:E + S], sym[pos])
    assert np.array_equal(_load(a, "decoded_block_sums_rank1"), _block_sums(sym))
    assert _load(a, "decoded_length_rank1").tolist() == [n]
    # the same output twice: the same arrays, element for element
    for k in ("decoded_length_rank1", "decoded_symbols_rank1", "decoded_block_sums_rank1"):
        assert np.array_equal(_load(a, k), _load(b, k))
    # a changed symbol anywhere shows in the block sums
    buf2 = buf.clone()
    i = int(pos[0]) + 1 if int(pos[0]) + 1 not in set(pos.tolist()) else 2 * E + 1
    buf2[i] ^= 1
    bench.dump_outputs(str(b), buf2, n, "_rank1")
    assert not np.array_equal(_load(a, "decoded_block_sums_rank1"), _load(b, "decoded_block_sums_rank1"))
    # at most 64 MB for any size
    assert 4 * (2 * E + S) + 8 * ((1 << 32) // bench.DUMP_BLOCK + 2) <= 64 * 10**6
