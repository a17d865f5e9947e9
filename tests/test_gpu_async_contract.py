"""The decode entry points' contract (include/hiphuff.h, hh_decode_device_async
and hh_decode_device_range_async): what each of hh_decode_device, _async,
_range and _range_async returns, when out_len and the range results are
filled, which failures are the call's and which are hh_decode_wait's, and
what hh_decoder_stats describes after a mix of them.  Small inputs only:
paper1.huff (17 tiles) and the first 40,001 bits of E.coli.huff (a 2-bit
code cut inside a code, so the tail rule applies)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -1, -5
ECOLI_BITS = 40_001


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


def _cut(hf, bits):
    """The oracle's decode of the first `bits` bits of a loaded .huff."""
    h = O.Huff(bits, 0, np.asarray(hf.izero, np.int32), np.asarray(hf.ione, np.int32),
               np.asarray(hf.sym, np.uint8), np.asarray(hf.data, np.uint8)[: (bits + 7) // 8])
    return O.OracleHuff.from_arrays(h).chain_decode()


def _dev(hh, data, bits):
    import torch
    buf = np.zeros((bits + 7) // 8 + hh.PAYLOAD_PAD, np.uint8)
    buf[: (bits + 7) // 8] = np.asarray(data, np.uint8)[: (bits + 7) // 8]
    return torch.from_numpy(buf).cuda()


def _out(n, fill=0xAB):
    import torch
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


def _clean(t, fill=0xAB):
    return int(t.ne(fill).sum()) == 0


def _async(hh, dec, d_in, bits, out, n):
    """hh_decode_device_async, raw: its return value (n: the caller's c_uint64)."""
    return hh.lib().hh_decode_device_async(dec._h, d_in.data_ptr(), bits, out.data_ptr(), out.numel(),
                                           C.byref(n), None)


def _wait_status(hh, dec):
    try:
        dec.wait()
    except hh.HipHuffError as e:
        return e.status
    return 0


@pytest.fixture(scope="module")
def paper1(hh, files_dir):
    path = os.path.join(files_dir, "paper1.huff")
    hf = hh.HuffFile.load(path)
    return hf, O.OracleHuff.load(path).chain_decode()


@pytest.fixture(scope="module")
def ecoli(hh, files_dir):
    hf = hh.HuffFile.load(os.path.join(files_dir, "E.coli.huff"))
    return hf, _cut(hf, ECOLI_BITS)


def test_fixed_async_capacity(hh, ecoli):
    """k_fixed, asynchronous, too small a buffer: the call returns HH_OK with
    the full length already in out_len and nothing written; the failure is
    the wait's, once; the next decode is unaffected."""
    import torch
    hf, ref = ecoli
    assert len(ref) == (ECOLI_BITS + 1) // 2
    dec = hh.Decoder(0)
    try:
        dec.set_tree(hf.tree())
        d_in = _dev(hh, hf.data, ECOLI_BITS)
        small = _out(len(ref) // 2)
        n = C.c_uint64(0)
        assert _async(hh, dec, d_in, ECOLI_BITS, small, n) == 0
        assert n.value == len(ref)
        torch.cuda.synchronize()
        assert _clean(small)
        assert _wait_status(hh, dec) == ERR_CAPACITY
        assert n.value == len(ref) and _clean(small)
        dec.wait()                                      # (cleared)
        big = _out(len(ref) + 64)
        m = dec.decode_device_async(d_in, ECOLI_BITS, big)
        dec.wait()
        assert dec.stats()["fixed_length"] == 1
        assert m.value == len(ref)
        assert np.array_equal(big[: m.value].cpu().numpy(), ref)
        assert _clean(big[m.value:])
    finally:
        dec.close()


def test_legacy_async_decodes_inside_the_call(hh, paper1):
    """A path that is not asynchronous (round 2's pipeline): the decode is
    done when hh_decode_device_async returns; a capacity failure is still
    the wait's, and the call returns HH_OK."""
    hf, ref = paper1
    dec = hh.Decoder(0, flags=hh.FLAG_LEGACY)
    try:
        dec.set_tree(hf.tree())
        d_in = _dev(hh, hf.data, hf.bits)
        out = _out(len(ref) + 64)
        n = C.c_uint64(0)
        assert _async(hh, dec, d_in, hf.bits, out, n) == 0
        assert n.value == len(ref)                      # (no wait yet)
        assert np.array_equal(out[: n.value].cpu().numpy(), ref)
        assert _clean(out[n.value:])
        assert dec.stats()["state_machine"] == 0
        dec.wait()
        small = _out(len(ref) // 2)
        m = C.c_uint64(0)
        assert _async(hh, dec, d_in, hf.bits, small, m) == 0
        assert m.value == len(ref)
        assert _wait_status(hh, dec) == ERR_CAPACITY
        dec.wait()
    finally:
        dec.close()


def test_legacy_range_async_decodes_inside_the_call(hh, paper1):
    """hh_decode_device_range_async on that path: the range's results are
    complete on return; a capacity failure returns HH_OK and is the wait's."""
    hf, ref = paper1
    dec = hh.Decoder(0, flags=hh.FLAG_LEGACY)
    try:
        dec.set_tree(hf.tree())
        tb = dec.tile_bits()
        assert hf.bits > 5 * tb
        d_in = _dev(hh, hf.data, hf.bits)
        out = _out(len(ref) + 64)
        want = dec.decode_range_ptr(d_in.data_ptr(), 5 * tb, 4, 0, out.data_ptr(), out.numel())
        assert 0 < want["out_len"] < len(ref)
        out.fill_(0xAB)
        r = dec.decode_range_async_ptr(d_in.data_ptr(), 5 * tb, 4, 0, out.data_ptr(), out.numel())
        got = r.as_dict()                               # (no wait yet)
        assert got == want
        assert np.array_equal(out[: got["out_len"]].cpu().numpy(), ref[: got["out_len"]])
        assert _clean(out[got["out_len"]:])
        dec.wait()
        small = _out(got["out_len"] // 2)
        dec.decode_range_async_ptr(d_in.data_ptr(), 5 * tb, 4, 0, small.data_ptr(), small.numel())   # (HH_OK)
        assert _wait_status(hh, dec) == ERR_CAPACITY
        dec.wait()
    finally:
        dec.close()


def test_argument_failures_are_the_calls(hh, paper1):
    """HH_ERR_ARG is returned by the call itself, with nothing launched and
    nothing pending: an entering state that is no state of the tree
    (ranges), a payload address that is no multiple of 4 (all four entry
    points)."""
    import torch
    hf, ref = paper1
    dec = hh.Decoder(0)
    try:
        dec.set_tree(hf.tree())
        tb = dec.tile_bits()
        d_in = _dev(hh, hf.data, hf.bits)
        out = _out(len(ref) + 64)
        p, o, cap = d_in.data_ptr(), out.data_ptr(), out.numel()
        nstates = int((np.asarray(hf.izero) >= 0).sum())          # (the tree's internal nodes)
        calls = []
        for s in (nstates, 1 << 16):
            calls.append(lambda s=s: dec.decode_range_async_ptr(p, 5 * tb, 4, s, o, cap))
            calls.append(lambda s=s: dec.decode_range_ptr(p, 5 * tb, 4, s, o, cap))
        for off in (1, 2):
            calls.append(lambda off=off: dec.decode_device_ptr(p + off, hf.bits - 64, o, cap))
            calls.append(lambda off=off: dec.decode_device_async(d_in[off:], hf.bits - 64, out))
            calls.append(lambda off=off: dec.decode_range_ptr(p + off, 5 * tb, 4, 0, o, cap))
            calls.append(lambda off=off: dec.decode_range_async_ptr(p + off, 5 * tb, 4, 0, o, cap))
        for k, call in enumerate(calls):
            with pytest.raises(hh.HipHuffError) as ei:
                call()
            assert ei.value.status == ERR_ARG, k
            dec.wait()                                  # (nothing pending, nothing kept)
        torch.cuda.synchronize()
        assert _clean(out)
        # the decoder still decodes
        n = dec.decode_device_async(d_in, hf.bits, out)
        dec.wait()
        assert n.value == len(ref) and np.array_equal(out[: n.value].cpu().numpy(), ref)
    finally:
        dec.close()


def test_stats_describe_the_last_decode_checked(hh, paper1):
    """async, async, wait: the stats are the last decode's.  async, then a
    synchronous decode: the stats are the synchronous one's, and the pending
    decode's failure is still the wait's."""
    hf, ref = paper1
    dec = hh.Decoder(0)
    try:
        dec.set_tree(hf.tree())
        tb = dec.tile_bits()
        cut = 3 * tb + 5
        ref_cut = _cut(hf, cut)
        assert 0 < len(ref_cut) < len(ref)
        d_in = _dev(hh, hf.data, hf.bits)
        o1, o2 = _out(len(ref) + 64), _out(len(ref) + 64)
        dec.decode_device_async(d_in, cut, o1)
        n2 = dec.decode_device_async(d_in, hf.bits, o2)
        dec.wait()
        st = dec.stats()
        assert st["state_machine"] in (1, 2) and st["out_len"] == len(ref) == n2.value
        small = _out(len(ref) // 2)
        dec.decode_device_async(d_in, hf.bits, small)
        assert dec.decode_device(d_in, cut, o1) == len(ref_cut)
        st = dec.stats()
        assert st["state_machine"] in (1, 2) and st["out_len"] == len(ref_cut)
        assert np.array_equal(o1[: len(ref_cut)].cpu().numpy(), ref_cut)
        assert _wait_status(hh, dec) == ERR_CAPACITY
        dec.wait()
    finally:
        dec.close()


def test_empty_input_checks_the_pending_decode(hh, paper1):
    """bits == 0 through hh_decode_device_async with a decode pending: the
    pending one is checked inside the call, which returns HH_OK, out_len 0."""
    hf, ref = paper1
    dec = hh.Decoder(0)
    try:
        dec.set_tree(hf.tree())
        d_in = _dev(hh, hf.data, hf.bits)
        out, other = _out(len(ref) + 64), _out(64)
        n = dec.decode_device_async(d_in, hf.bits, out)
        m = C.c_uint64(7)
        assert _async(hh, dec, d_in, 0, other, m) == 0
        assert m.value == 0
        assert n.value == len(ref)                      # (checked by that call, no wait yet)
        assert np.array_equal(out[: n.value].cpu().numpy(), ref)
        assert _clean(other)
        dec.wait()
    finally:
        dec.close()
