"""hh_histogram_device in stream order (this project has had a null-stream
race before): the input is filled by torch ops on a non-default stream and
counted on the same stream with no sync in between.

In a file of its own, after the other GPU files in collection order, because
it is the one new test that puts work on a side stream: the first use of a
side stream changes which hardware queue later streams get, and
tests/test_gpu_one.py::test_single_pass_two_decoders_two_streams is
sensitive to that (it refills its outputs on the null stream between
decodes on two non-blocking streams)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_histogram_stream_order():
    import torch
    import huffmandecoderongpus_amd as H
    n = 32 << 20
    enc = H.Encoder(0)
    try:
        st = torch.cuda.Stream()
        d = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for _ in range(4):                      # (work queued ahead of the histogram)
                d.add_(1)
            d[: n // 2] = 200
            got = enc.histogram(d, st)
    finally:
        enc.close()
    want = np.zeros(256, np.uint64)
    want[4], want[200] = n - n // 2, n // 2
    assert np.array_equal(got, want)
