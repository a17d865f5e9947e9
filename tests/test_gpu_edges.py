"""The decoder at the stream lengths where its launch changes shape, at
exact capacities and at misaligned pointers (tests/edge_cases.py has the
lengths and the codes; tests/test_emu_edges.py::test_fsm_launch_breakpoints
runs the same lengths through the emulator).

Every output buffer is filled with 0xAB first and the decoder gets a view of
it: a byte stored outside that view shows in the bytes around it, which an
output tensor of exactly `cap` bytes (the allocator's slack behind it) would
hide.  All comparisons are byte-exact against the oracle's chain decode of
the same prefix of one stream per code."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import pytest

import edge_cases as E

pytestmark = pytest.mark.gpu

GUARD = 4096
DEFAULT_M = 2              # HH_CNT_M (csrc/hh_fsm.hip); test_launch_breakpoints checks it
ERR_ARG, ERR_CAPACITY = -1, -5
_REFS = {}                 # (code, bits) -> the oracle's decode, on the GPU


@pytest.fixture(scope="module")
def hh():
    import huffmandecoderongpus_amd as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _drop_refs():
    yield
    import torch
    _REFS.clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def two_pass(monkeypatch):
    monkeypatch.setenv("HH_ONE", "0")           # (fsm_launch's own kernels; read when the tree is set)
    monkeypatch.delenv("HH_CNT_M", raising=False)


def _refs(name, data, cuts):
    """The oracle's decodes of the prefixes `cuts`, each computed once (a
    few at a time: the oracle keeps no state) and kept on the GPU."""
    import torch
    c = E.code(name)
    miss = [b for b in dict.fromkeys(cuts) if (name, b) not in _REFS]
    if miss:
        with ThreadPoolExecutor(8) as ex:
            for b, r in zip(miss, ex.map(lambda b: E.oracle_prefix(c, data, b), miss)):
                _REFS[(name, b)] = torch.from_numpy(r).cuda()
    return {b: _REFS[(name, b)] for b in cuts}


def _decoder(hh, name, flags=None):
    c = E.code(name)
    dec = hh.Decoder(0, flags=c.flags if flags is None else flags)
    dec.set_tree(c.tree())
    return dec


def _abi(hh, dec, d_data, bits, d_out, cap, fn="hh_decode_device"):
    """(rc, out_len) of the C ABI's decode on the default stream."""
    n = C.c_uint64(0)
    rc = getattr(hh.lib(), fn)(dec._h, d_data, bits, d_out, cap, C.byref(n), None)
    return rc, int(n.value)


def _clean(t):
    return bool(t.eq(0xAB).all().item())


def _two_pass_ran(st):
    return st["state_machine"] == 1 and st["exact_fallback"] == 0 and st["fixed_length"] == 0


@pytest.mark.parametrize("M", [None, "1", "4"])
@pytest.mark.parametrize("name", E.CODE_NAMES)
def test_launch_breakpoints(hh, name, M, monkeypatch):
    """Every length of edge_cases.breakpoint_bits -- both sides of each
    inequality fsm_launch chooses its kernels and grids by, for the default
    HH_CNT_M, 1 and 4 -- decoded into exactly the oracle's length: the bytes
    are the oracle's, nothing is written past them, and the state machine's
    two passes did it.  The rows k = 1023..2049 tiles are the scan of two and
    three k_fscan1 blocks (each tile's base is blk[t / 1024] plus its prefix
    within the block: the comment at k_fscan1's fscan_block points here)."""
    import torch
    if M is not None:
        monkeypatch.setenv("HH_CNT_M", M)
    dec = _decoder(hh, name)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        assert TB == 64 * S and S % 32 == 0 and (name != "byte256" or S == 224)
        data, bits, _ = E.stream(name, S)
        d_data = torch.from_numpy(data).cuda()
        m = int(M) if M is not None else DEFAULT_M
        cuts = E.breakpoint_bits(S, m, dec._tree.info()["maxlen"], bits)
        assert cuts[-1] == 2049 * TB + S + 1 and {1024 * TB, 2048 * TB, TB + S + 1} <= set(cuts)
        refs = _refs(name, data, cuts)
        buf = torch.empty(max(r.numel() for r in refs.values()) + GUARD, dtype=torch.uint8, device="cuda")
        if M is None:
            # the default's regions per lane: a segment's leave state is proven
            # independent of its entry from more than HH_CNT_M tiles on
            seen = [dec.decode_range_ptr(d_data.data_ptr(), bits, k, 0, buf.data_ptr(), buf.numel())["const_seen"]
                    for k in (DEFAULT_M, DEFAULT_M + 1)]
            assert seen == [False, True], seen
        for cut in cuts:
            ref = refs[cut]
            n = ref.numel()
            buf[: n + GUARD].fill_(0xAB)
            rc, got = _abi(hh, dec, d_data.data_ptr(), cut, buf.data_ptr(), n)
            where = (cut, divmod(cut, TB), n)
            assert rc == 0 and got == n, (rc, got, where)
            assert torch.equal(buf[:n], ref), where
            assert _clean(buf[n: n + GUARD]), where
            assert _two_pass_ran(dec.stats()), (dec.stats(), where)
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["kjv", "byte256"])
def test_range_breakpoints(hh, name):
    """Two segments of a 6-tile stream (plus S + 1 bits; and of exactly 6
    tiles), split after every tile t = 1..5, the second entered after a
    prologue of 0, 1 and 2 tiles: it finds the first's leave state, and the
    outputs, each decoded into a capacity with nothing to spare, concatenate
    to the oracle's."""
    import torch
    dec = _decoder(hh, name)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        data, _, _ = E.stream(name, S)
        d_data = torch.from_numpy(data).cuda()
        refs = _refs(name, data, [6 * TB + S + 1, 6 * TB])
        for bits, ref in refs.items():
            total = ref.numel()
            a = torch.empty(total + GUARD, dtype=torch.uint8, device="cuda")
            b = torch.empty(total + GUARD, dtype=torch.uint8, device="cuda")
            for t in range(1, 6):
                a.fill_(0xAB)
                ra = dec.decode_range_ptr(d_data.data_ptr(), bits, t, 0, a.data_ptr(), total)
                assert _two_pass_ran(dec.stats())
                na = ra["out_len"]
                assert 0 < na < total and _clean(a[na:]), (bits, t, na)
                assert torch.equal(a[:na], ref[:na]), (bits, t)
                for p in (0, 1, 2):
                    if p > t:
                        continue
                    b0 = (t - p) * TB
                    left = bits - b0
                    b.fill_(0xAB)
                    rb = dec.decode_range_ptr(d_data.data_ptr() + b0 // 8, left, (left + TB - 1) // TB,
                                              ra["leave_state"] if p == 0 else 0, b.data_ptr(), total - na,
                                              prologue=p)
                    where = (bits, t, p, ra, rb)
                    assert _two_pass_ran(dec.stats()), where
                    assert rb["entry_state"] == ra["leave_state"], where
                    assert rb["out_len"] == total - na, where
                    assert torch.equal(b[: total - na], ref[na:]), where
                    assert _clean(b[total - na:]), where
    finally:
        dec.close()


_PATHS = {
    # path: (code, decoder flags, what stats() must say, lengths it takes)
    "fsm-kjv": ("kjv", 0, _two_pass_ran, 3),
    "fsm-fixed2": ("fixed2", E.FLAG_NO_FIXED, _two_pass_ran, 3),
    "k_fixed": ("fixed2", 0, lambda st: st["fixed_length"] == 1, 3),
    "legacy": ("kjv", 8, lambda st: st["state_machine"] == 0 and st["exact_fallback"] == 0, 3),
    "segment": ("kjv", 2, lambda st: st["exact_fallback"] == 2, 3),
    "exact": ("kjv", 1, lambda st: st["exact_fallback"] == 1, 1),
    "async": ("kjv", 0, _two_pass_ran, 3),
}


@pytest.mark.parametrize("path", list(_PATHS))
def test_capacity_is_a_hard_bound(hh, path):
    """Every decode path at a capacity of exactly the stream's symbols n
    (rc 0, the oracle's bytes), n - 1, the symbols before the last tile and 0
    (HH_ERR_CAPACITY, out_len = n): nothing at or beyond d_out + cap is
    written.  Streams of one tile less 3 bits, (M + 1) tiles + S + 1 bits and
    1025 tiles + 1 bit (FORCE_EXACT: the first only)."""
    import torch
    name, flags, took, nlen = _PATHS[path]
    L = hh.lib()
    dec = _decoder(hh, name, flags)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        data, _, _ = E.stream(name, S)
        d_data = torch.from_numpy(data).cuda()
        lengths = [TB - 3, (DEFAULT_M + 1) * TB + S + 1, 1025 * TB + 1][:nlen]
        before = {b: (b + TB - 1) // TB * TB - TB for b in lengths}      # without the last tile
        refs = _refs(name, data, lengths + list(before.values()))

        def decode(bits, d_out, cap):
            if path != "async":
                return _abi(hh, dec, d_data.data_ptr(), bits, d_out, cap)
            n = C.c_uint64(0)
            rc = L.hh_decode_device_async(dec._h, d_data.data_ptr(), bits, d_out, cap, C.byref(n), None)
            assert rc == 0, rc                    # (enqueued; a capacity failure is hh_decode_wait's)
            return L.hh_decode_wait(dec._h), int(n.value)

        for bits in lengths:
            ref = refs[bits]
            n = ref.numel()
            buf = torch.empty(n + GUARD, dtype=torch.uint8, device="cuda")
            caps = [n, n - 1, refs[before[bits]].numel(), 0]
            assert caps[2] < n
            for cap in caps:
                buf.fill_(0xAB)
                rc, got = decode(bits, buf.data_ptr(), cap)
                torch.cuda.synchronize()
                where = (path, bits, cap, n, rc, got)
                assert _clean(buf[cap:]), where
                if cap == n:
                    assert rc == 0 and got == n, where
                    assert torch.equal(buf[:n], ref), where
                    assert took(dec.stats()), (dec.stats(), where)
                else:
                    assert rc == ERR_CAPACITY and got == n, where
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["kjv", "byte256", "fixed2"])
def test_pointer_alignment(hh, name):
    """The output at every address mod 16 (k_emf rounds its 16-byte stores by
    the offset inside the output, so all of them are unaligned then) and the
    payload at 0, 4, 8 and 12 mod 16 (word loads), at 3 tiles + S + 1 bits
    and 1025 tiles + 1 bit: the oracle's bytes, none before or behind them.
    A payload off a 4-byte boundary is refused (HH_ERR_ARG) before anything
    is launched."""
    import torch
    dec = _decoder(hh, name)
    try:
        TB = dec.tile_bits()
        S = TB // 64
        data, _, _ = E.stream(name, S)
        lengths = [3 * TB + S + 1, 1025 * TB + 1]
        refs = _refs(name, data, lengths)
        nb = (lengths[-1] + 7) // 8 + hh.PAYLOAD_PAD
        pbuf = torch.zeros(16 + nb, dtype=torch.uint8, device="cuda")
        host = torch.from_numpy(data[:nb]).cuda()
        assert pbuf.data_ptr() % 16 == 0
        for q in range(4):
            pbuf.zero_()
            pay = pbuf[4 * q: 4 * q + nb]
            pay.copy_(host)
            assert pay.data_ptr() % 16 == 4 * q
            for bits in lengths:
                ref = refs[bits]
                n = ref.numel()
                buf = torch.empty(16 + n + GUARD, dtype=torch.uint8, device="cuda")
                assert buf.data_ptr() % 16 == 0
                for off in range(16):
                    buf.fill_(0xAB)
                    out = buf[off: off + n]
                    assert out.data_ptr() % 16 == off
                    rc, got = _abi(hh, dec, pay.data_ptr(), bits, out.data_ptr(), n)
                    where = (name, q, bits, off, rc, got, n)
                    assert rc == 0 and got == n, where
                    assert torch.equal(out, ref), where
                    assert _clean(buf[:off]) and _clean(buf[off + n:]), where
                    assert _two_pass_ran(dec.stats()), where
        # a payload off a word boundary: refused, nothing launched
        buf.fill_(0xAB)
        for off in (1, 2, 3):
            for fn in ("hh_decode_device", "hh_decode_device_async"):
                rc, got = _abi(hh, dec, pbuf.data_ptr() + off, lengths[0], buf.data_ptr(), buf.numel(), fn)
                assert rc == ERR_ARG and got == 0, (off, fn, rc, got)
        assert hh.lib().hh_decode_wait(dec._h) == 0
        torch.cuda.synchronize()
        assert _clean(buf)
    finally:
        dec.close()
