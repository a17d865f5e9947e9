"""The edge cases of tests/edge_cases.py on the host: fsm_launch's
breakpoints through the kernel emulator, and the host encoder (the reference
the device encoder is compared with) on codes of up to 64 bits."""
import numpy as np
import pytest

import huffmandecoderongpus_amd as H
from oracle import oracle as O
from test_emu import femu, run_femu   # noqa: F401  (femu: the emulator fixture)


# ---------------------------------------------------------------------------
# fsm_launch's breakpoints (tests/edge_cases.py), on the host: the list
# tests/test_gpu_edges.py decodes on the GPU, through the emulator.  A length
# that fails here is wrong in the algorithm (or in the list); one that fails
# only on the GPU is wrong in a kernel or in the launch.
# ---------------------------------------------------------------------------
_BP_TILES = 1025
_bp_refs = {}                                # (code, bits) -> the oracle's decode


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("name", ["kjv", "byte256", "caterpillar40"])
def test_fsm_launch_breakpoints(femu, name, M):
    """edge_cases.breakpoint_bits(S, M, maxlen) with the rows k <= 33 whole
    and, around the scan blocks, k in {1023, 1024, 1025} with every offset
    d in {-1, 0, 1, S, S + 1} (nothing thinned): each prefix of one stream of
    kjv's tree, the 256-leaf byte-alphabet tree and the 40-deep caterpillar,
    M in {1, 2, 4} regions per lane, against the oracle's decode of the same
    prefix.  S (and the head) come from the emulator's own table builder."""
    import edge_cases as E
    c = E.code(name)
    try:
        _, _, st, _, _ = run_femu(femu, c.izero, c.ione, c.sym, np.zeros(8, np.uint8), 40, M=M)
        S = int(st[3])
        assert S % 32 == 0 and (name != "byte256" or S == 224)
        data, bits, _ = E.stream(name, S, _BP_TILES)
        cuts = E.breakpoint_bits(S, M, c.tree().info()["maxlen"], bits, scan_k=(1023, 1024, 1025))
        assert cuts[-1] == 1025 * 64 * S + S + 1 and 1024 * 64 * S in cuts      # the rows are all there
        for cut in cuts:
            ref = _bp_refs.get((name, cut))
            if ref is None:
                ref = _bp_refs[(name, cut)] = E.oracle_prefix(c, data, cut)
            n, out, st, _, _ = run_femu(femu, c.izero, c.ione, c.sym, data, cut, M=M)
            assert n == len(ref) and np.array_equal(out, ref), (cut, divmod(cut, 64 * S), n, len(ref), st)
    finally:
        femu.hh_fsm_emu_set_m(1)              # (the library's setting outlives the test)


def test_host_encoder_every_offset_and_length():
    """The host encoder (the reference the device encoder is compared with)
    on codes of 1..64 bits, each starting at every bit offset 0..31 of a
    32-bit word (edge_cases.every_offset_text: all 2048 pairs, codes over one,
    two and three words): the oracle decodes its stream back to the text."""
    import edge_cases as E
    iz, io, sy, text = E.every_offset_text(64)
    tree = H.Tree(iz, io, sy)
    assert tree.info()["maxlen"] == 64
    data, bits = tree.encode(text)
    assert bits == int((text.astype(np.int64) + 1).sum())
    hf = O.Huff(bits, 0, np.asarray(iz, np.int32), np.asarray(io, np.int32), np.asarray(sy, np.uint8),
                data[: (bits + 7) // 8])
    back = O.OracleHuff.from_arrays(hf).chain_decode()
    assert len(back) == len(text) and np.array_equal(back, text)
    assert not data[(bits + 7) // 8:].any()          # nothing past the stream's last byte
