"""hiphuff -- MI355X-native parallel Huffman decoder (Python host binding).

A thin ctypes layer over the C ABI in ``include/hiphuff.h`` (the library
``libhiphuff.so`` in this package directory, built by the top-level
Makefile).  The decode itself always runs in the HIP kernels; there is no CPU
fallback in this package -- if the library (or a GPU) is missing, the calls
raise.

Mirrors the reference's plugin interface (framework/decodeUtil.h:14-19): a
``Decoder`` is the device state behind one decoder function, ``decode_host``
is the evaluate()-timed scope (H2D + decode + D2H, decodeUtil.c:41-43) and
``decode_device`` is the HBM-resident hot path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# HIPHUFF_LIB overrides the library (diagnostic builds, e.g. build/libhiphuff_stamps.so)
LIB_PATH = os.environ.get("HIPHUFF_LIB") or os.path.join(HERE, "libhiphuff.so")
PAYLOAD_PAD = 64   # HH_PAYLOAD_PAD

_ERRORS = {
    0: "ok", -1: "bad argument", -2: "i/o error", -3: "not a HUFF/HUFX file",
    -4: "invalid code tree", -5: "output buffer too small", -6: "HIP runtime error",
    -7: "out of memory", -8: "internal error", -9: "in-kernel wait timed out",
    -10: "unsupported input",
}


class HipHuffError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__(f"{what}: {_ERRORS.get(status, status)} ({status})")


class _Huff(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("izero", C.POINTER(C.c_int32)),
                ("ione", C.POINTER(C.c_int32)), ("sym", C.POINTER(C.c_uint8)),
                ("bits", C.c_uint64), ("uncompressedsize", C.c_uint64),
                ("data", C.POINTER(C.c_uint8)), ("wide", C.c_int)]


class _Tree(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("izero", C.c_void_p), ("ione", C.c_void_p),
                ("sym", C.c_void_p)]


BUILD_MAX_NODES = 511   # HH_BUILD_MAX_NODES


class _TreeBuf(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("izero", C.c_int32 * BUILD_MAX_NODES),
                ("ione", C.c_int32 * BUILD_MAX_NODES), ("sym", C.c_uint8 * BUILD_MAX_NODES)]


class _TreeInfo(C.Structure):
    _fields_ = [("reachable", C.c_int32), ("leaves", C.c_int32), ("minlen", C.c_int32),
                ("maxlen", C.c_int32), ("len_gcd", C.c_int32)]


class _Config(C.Structure):
    _fields_ = [("device", C.c_int), ("lane_bits", C.c_int), ("flags", C.c_int)]


class _Stats(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_sync", C.c_double), ("ms_scan", C.c_double),
                ("ms_emit", C.c_double), ("out_len", C.c_uint64), ("lanes", C.c_uint64),
                ("repairs", C.c_uint64), ("exact_fallback", C.c_int), ("fixed_length", C.c_int),
                ("state_machine", C.c_int)]


class _Range(C.Structure):
    _fields_ = [("bits_avail", C.c_uint64), ("ntiles", C.c_uint64), ("prologue", C.c_uint64),
                ("in_state", C.c_uint32)]


class _RangeOut(C.Structure):
    _fields_ = [("out_len", C.c_uint64), ("leave_state", C.c_uint32), ("const_seen", C.c_uint32),
                ("entry_state", C.c_uint32), ("entry_exact", C.c_uint32)]


FLAG_FORCE_EXACT = 1
FLAG_FORCE_SEGMENT = 2
FLAG_NO_FIXED = 4     # HH_FLAG_NO_FIXED: fixed-length codes through the general pipeline too
FLAG_LEGACY = 8       # HH_FLAG_LEGACY: round 2's pipeline instead of the state-machine decode
FLAG_PHASE_TIMING = 16  # HH_FLAG_PHASE_TIMING: events between the kernels (ms_sync/scan/emit)
FLAG_KEEP_HOST_PINNED = 32  # HH_FLAG_KEEP_HOST_PINNED: decode_host keeps the caller's buffers page-locked
FLAG_TWO_PASS = 64    # HH_FLAG_TWO_PASS: the state machine's two-pass form instead of its single pass
_lib_handle: Optional[C.CDLL] = None

# exported symbols and their ctypes signatures; tests check every one of these
# against include/hiphuff.h
_SIGS = {
    "hh_strerror": ([C.c_int], C.c_char_p),
    "hh_tree_check": ([C.POINTER(_Tree), C.POINTER(_TreeInfo)], C.c_int),
    "hh_huff_load": ([C.c_char_p, C.POINTER(_Huff)], C.c_int),
    "hh_huff_save": ([C.c_char_p, C.POINTER(_Huff)], C.c_int),
    "hh_huff_free": ([C.POINTER(_Huff)], None),
    "hh_huff_tree": ([C.POINTER(_Huff)], _Tree),
    "hh_encode_bound": ([C.POINTER(_Tree), C.c_uint64], C.c_uint64),
    "hh_encode": ([C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_void_p,
                   C.POINTER(C.c_uint64)], C.c_int),
    "hh_encode_device": ([C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                          C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_encoder_create": ([C.POINTER(C.c_void_p), C.c_int], C.c_int),
    "hh_encoder_destroy": ([C.c_void_p], None),
    "hh_encoder_encode": ([C.c_void_p, C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                           C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_tree_build": ([C.POINTER(C.c_uint64), C.POINTER(_TreeBuf)], C.c_int),
    "hh_histogram_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_compress_bound": ([C.c_uint64], C.c_uint64),
    "hh_compress_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(_TreeBuf),
                            C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_encode_blocks_bound": ([C.POINTER(_Tree), C.c_uint64, C.c_uint64], C.c_uint64),
    "hh_encode_blocks": ([C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                          C.POINTER(C.c_uint64)], C.c_int),
    "hh_encoder_encode_blocks": ([C.c_void_p, C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                  C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_compress_blocks_bound": ([C.c_uint64, C.c_uint64], C.c_uint64),
    "hh_compress_blocks_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.POINTER(_TreeBuf), C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_encoder_encode_blocks_items": ([C.c_void_p, C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p],
                                       C.c_int),
    "hh_compress_blocks_device_items": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.POINTER(_TreeBuf), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                         C.c_void_p], C.c_int),
    "hh_encode_ragged_bound": ([C.POINTER(_Tree), C.c_uint64, C.c_uint64], C.c_uint64),
    "hh_encode_ragged": ([C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                          C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hh_encoder_encode_ragged": ([C.c_void_p, C.POINTER(_Tree), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p],
                                 C.c_int),
    "hh_compress_ragged_bound": ([C.c_uint64, C.c_uint64], C.c_uint64),
    "hh_compress_ragged_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.POINTER(_TreeBuf), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p],
                                  C.c_int),
    "hh_decoder_create": ([C.POINTER(C.c_void_p), C.POINTER(_Config)], C.c_int),
    "hh_decoder_destroy": ([C.c_void_p], None),
    "hh_decoder_set_tree": ([C.c_void_p, C.POINTER(_Tree)], C.c_int),
    "hh_decoder_stats": ([C.c_void_p, C.POINTER(_Stats)], C.c_int),
    "hh_decode_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                          C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_decode_device_async": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hh_decode_wait": ([C.c_void_p], C.c_int),
    "hh_decode_batch_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.c_void_p], C.c_int),
    "hh_decode_batch_device_items": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hh_decode_blocks_read": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                              C.c_int),
    "hh_decode_blocks_gather": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                 C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
                                C.c_int),
    "hh_decode_batch_take": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hh_decode_take_round_tiles": ([C.c_void_p, C.POINTER(C.c_uint32)], C.c_int),
    "hh_decode_batch_round_tiles": ([C.c_void_p, C.POINTER(C.c_uint32)], C.c_int),
    "hh_decoder_tile_bits": ([C.c_void_p, C.POINTER(C.c_uint64)], C.c_int),
    "hh_decode_device_range": ([C.c_void_p, C.c_void_p, C.POINTER(_Range), C.c_void_p,
                                C.c_uint64, C.POINTER(_RangeOut), C.c_void_p], C.c_int),
    "hh_decode_device_range_async": ([C.c_void_p, C.c_void_p, C.POINTER(_Range), C.c_void_p,
                                      C.c_uint64, C.POINTER(_RangeOut), C.c_void_p], C.c_int),
    "hh_decoder_release_host": ([C.c_void_p], C.c_int),
    "hh_decode_host": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                        C.POINTER(C.c_uint64)], C.c_int),
    "hh_copy_device": ([C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                        C.POINTER(C.c_float)], C.c_int),
    "hh_stage_initbitsindex": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p], C.c_int),
    "hh_stage_decodeallbits": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p], C.c_int),
    "hh_stage_makebigtable": ([C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                               C.POINTER(C.c_int32), C.c_void_p], C.c_int),
    "hh_stage_calcbitsindex": ([C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p], C.c_int),
    "hh_stage_calcresult": ([C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p], C.c_int),
    "hh_stage_findmax": ([C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int32),
                          C.c_void_p], C.c_int),
    "hh_stage_pipeline": ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64,
                           C.POINTER(C.c_uint64), C.c_void_p], C.c_int),
    "hipHuffApproach": ([C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hh_debug_counters": ([C.c_void_p, C.c_void_p], C.c_int),
    "hh_debug_fsm": ([C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "hh_debug_geometry": ([C.c_void_p, C.POINTER(C.c_uint32)], C.c_int),
}


def lib() -> C.CDLL:
    """The HIP library; raises if it was not built (no silent fallback)."""
    global _lib_handle
    if _lib_handle is None:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7.
        # Loading torch first lets libhiphuff.so bind to that same runtime
        # (same soname), so device pointers and streams are shared with torch.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `make` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        # every declared symbol must be there; only an explicit A/B build
        # of an older revision (HIPHUFF_AB_BUILD=1, tools/mkrev.sh) may lack
        # some -- those are named on stderr and left unbound
        ab = os.environ.get("HIPHUFF_AB_BUILD") == "1"
        skipped = []
        for name, (args, res) in _SIGS.items():
            if ab and not hasattr(L, name):
                skipped.append(name)
                continue
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        if skipped:
            import sys
            print(f"hiphuff: {LIB_PATH} (HIPHUFF_AB_BUILD) lacks {', '.join(skipped)}", file=sys.stderr)
        _lib_handle = L
    return _lib_handle


def _check(rc: int, what: str):
    if rc != 0:
        raise HipHuffError(rc, what)


@dataclass
class HuffFile:
    """A .huff container (HUFF or 64-bit HUFX), huffdata.c:27-68."""
    izero: np.ndarray
    ione: np.ndarray
    sym: np.ndarray
    bits: int
    uncompressedsize: int
    data: np.ndarray       # payload + PAYLOAD_PAD zero bytes

    @property
    def nodes(self) -> int:
        return int(self.izero.shape[0])

    @property
    def payload(self) -> np.ndarray:
        return self.data[: (self.bits + 7) // 8]

    @classmethod
    def load(cls, path: str) -> "HuffFile":
        h = _Huff()
        _check(lib().hh_huff_load(path.encode(), C.byref(h)), f"load {path}")
        try:
            n = h.nodes
            iz = np.ctypeslib.as_array(h.izero, shape=(n,)).copy()
            io = np.ctypeslib.as_array(h.ione, shape=(n,)).copy()
            sy = np.ctypeslib.as_array(h.sym, shape=(n,)).copy()
            nb = (h.bits + 7) // 8 + PAYLOAD_PAD
            data = np.ctypeslib.as_array(h.data, shape=(nb,)).copy()
            return cls(iz, io, sy, int(h.bits), int(h.uncompressedsize), data)
        finally:
            lib().hh_huff_free(C.byref(h))

    def save(self, path: str, wide: bool = False):
        keep = [np.ascontiguousarray(self.izero, np.int32),
                np.ascontiguousarray(self.ione, np.int32),
                np.ascontiguousarray(self.sym, np.uint8),
                np.ascontiguousarray(self.data, np.uint8)]
        h = _Huff(self.nodes, keep[0].ctypes.data_as(C.POINTER(C.c_int32)),
                  keep[1].ctypes.data_as(C.POINTER(C.c_int32)),
                  keep[2].ctypes.data_as(C.POINTER(C.c_uint8)), self.bits,
                  self.uncompressedsize, keep[3].ctypes.data_as(C.POINTER(C.c_uint8)),
                  int(wide))
        _check(lib().hh_huff_save(path.encode(), C.byref(h)), f"save {path}")

    def tree(self) -> "Tree":
        return Tree(self.izero, self.ione, self.sym)


class Tree:
    """Code tree in the reference's node layout (huffdata.h:12-16), SoA."""

    def __init__(self, izero, ione, sym):
        self.izero = np.ascontiguousarray(izero, np.int32)
        self.ione = np.ascontiguousarray(ione, np.int32)
        self.sym = np.ascontiguousarray(sym, np.uint8)
        self._c = _Tree(len(self.izero), self.izero.ctypes.data, self.ione.ctypes.data,
                        self.sym.ctypes.data)

    @classmethod
    def _from_buf(cls, tb: "_TreeBuf") -> "Tree":
        n = tb.nodes
        return cls(np.array(tb.izero[:n], np.int32), np.array(tb.ione[:n], np.int32),
                   np.array(tb.sym[:n], np.uint8))

    @classmethod
    def from_counts(cls, counts) -> "Tree":
        """The Huffman tree of byte counts (hh_tree_build; up to 256 of them,
        the rest zero): node for node what synth.huffman_tree builds."""
        c = np.zeros(256, np.uint64)
        given = np.asarray(counts)
        if given.ndim != 1 or given.size > 256:
            raise ValueError("counts: a vector of at most 256 entries")
        if given.dtype.kind not in "ui":
            # (Python ints beyond int64 arrive as floats or objects: exact through int())
            vals = [int(v) for v in counts]
            if any(v != w for v, w in zip(vals, counts)):
                raise ValueError("counts: integers")
            given = np.array(vals, dtype=object)
        if given.size and (min(given.tolist()) < 0 or max(given.tolist()) >= 1 << 64):
            raise ValueError("counts: entries in [0, 2^64)")
        c[: given.size] = given.astype(np.uint64)
        tb = _TreeBuf()
        _check(lib().hh_tree_build(c.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(tb)), "tree build")
        return cls._from_buf(tb)

    def info(self) -> dict:
        inf = _TreeInfo()
        _check(lib().hh_tree_check(C.byref(self._c), C.byref(inf)), "tree check")
        return {k: getattr(inf, k) for k, _ in _TreeInfo._fields_}

    def encode(self, syms: np.ndarray) -> tuple[np.ndarray, int]:
        """Pack symbols LSB-first with this tree's codes -> (payload+pad, bits)."""
        syms = np.ascontiguousarray(syms, np.uint8)
        bound = lib().hh_encode_bound(C.byref(self._c), len(syms))
        if bound == 0:
            raise HipHuffError(-4, "encode bound")
        out = np.zeros(bound + PAYLOAD_PAD, np.uint8)
        bits = C.c_uint64(0)
        _check(lib().hh_encode(C.byref(self._c), syms.ctypes.data, len(syms), out.ctypes.data,
                               C.byref(bits)), "encode")
        nb = (bits.value + 7) // 8
        return out[: nb + PAYLOAD_PAD].copy(), int(bits.value)

    def encode_blocks(self, syms: np.ndarray, block_syms: int, cap: Optional[int] = None) -> tuple:
        """The host reference of the blocked encode (hh_encode_blocks): syms
        cut into blocks of block_syms, each encoded on its own and packed at
        4-byte boundaries -> (data + PAYLOAD_PAD zero bytes, items (nb, 4)
        uint64: data_off, bits, out_off, cap -- what Decoder.decode_batch
        takes).  cap: the output's capacity (default: encode_blocks_bound); a
        HipHuffError of status -5 carries .items and .total_bytes."""
        syms = np.ascontiguousarray(syms, np.uint8)
        n = len(syms)
        if cap is None:
            cap = encode_blocks_bound(self, n, block_syms) if block_syms > 0 else 0
        out = np.zeros(cap + PAYLOAD_PAD, np.uint8)
        items = np.zeros((_nblocks(n, block_syms), 4), np.uint64)
        total = C.c_uint64(0)
        rc = lib().hh_encode_blocks(C.byref(self._c), syms.ctypes.data, n, block_syms, out.ctypes.data, cap,
                                    items.ctypes.data, C.byref(total))
        if rc == -5:
            e = HipHuffError(rc, "encode_blocks")
            e.items, e.total_bytes = items, int(total.value)
            raise e
        _check(rc, "encode_blocks")
        return out[: total.value + PAYLOAD_PAD].copy(), items

    def encode_ragged(self, syms: np.ndarray, offsets, cap: Optional[int] = None) -> tuple:
        """The host reference of the ragged blocked encode (hh_encode_ragged):
        record r the symbols [offsets[r], offsets[r + 1]) (offsets[0] == 0,
        nondecreasing, offsets[-1] == len(syms); a record may be empty), each
        encoded on its own and packed at 4-byte boundaries -> (data +
        PAYLOAD_PAD zero bytes, items (nrec, 4) uint64: data_off, bits,
        out_off, cap).  cap: the output's capacity (default:
        encode_ragged_bound); a HipHuffError of status -5 carries .items and
        .total_bytes."""
        syms = np.ascontiguousarray(syms, np.uint8)
        offs = _ragged_offsets(offsets)
        n, nrec = len(syms), offs.size - 1
        if cap is None:
            cap = encode_ragged_bound(self, n, nrec)
        out = np.zeros(cap + PAYLOAD_PAD, np.uint8)
        items = np.zeros((nrec, 4), np.uint64)
        total = C.c_uint64(0)
        rc = lib().hh_encode_ragged(C.byref(self._c), syms.ctypes.data, n, offs.ctypes.data, nrec, out.ctypes.data, cap,
                                    items.ctypes.data, C.byref(total))
        if rc == -5:
            e = HipHuffError(rc, "encode_ragged")
            e.items, e.total_bytes = items, int(total.value)
            raise e
        _check(rc, "encode_ragged")
        return out[: total.value + PAYLOAD_PAD].copy(), items


def _ragged_offsets(offsets) -> np.ndarray:
    """A host offsets list as the uint64 (nrec + 1,) array the C calls take."""
    offs = np.ascontiguousarray(offsets)
    if offs.ndim != 1 or offs.size < 1 or offs.dtype.kind not in "ui":
        raise ValueError("offsets: a vector of nrec + 1 integers")
    return offs.astype(np.int64, copy=False).view(np.uint64) if offs.dtype.kind == "i" else \
        np.ascontiguousarray(offs, np.uint64)


def encode_ragged_bound(tree: "Tree", n: int, nrec: int) -> int:
    """hh_encode_ragged_bound: bytes that always hold the ragged stream of n
    symbols of tree in nrec records."""
    bound = int(lib().hh_encode_ragged_bound(C.byref(tree._c), n, nrec))
    if bound == 0 and (n or nrec):
        raise HipHuffError(-4, "encode_ragged bound")
    return bound


def compress_ragged_bound(n: int, nrec: int) -> int:
    """hh_compress_ragged_bound: bytes that always hold n symbols compressed
    in nrec records with their own Huffman code."""
    return int(lib().hh_compress_ragged_bound(n, nrec))


def _nblocks(n: int, block_syms: int) -> int:
    return -(-n // block_syms) if block_syms > 0 else 0


def encode_blocks_bound(tree: "Tree", n: int, block_syms: int) -> int:
    """hh_encode_blocks_bound: bytes that always hold the blocked stream of n
    symbols of tree."""
    bound = int(lib().hh_encode_blocks_bound(C.byref(tree._c), n, block_syms))
    if bound == 0 and n:
        raise HipHuffError(-4 if block_syms > 0 else -1, "encode_blocks bound")
    return bound


def compress_blocks_bound(n: int, block_syms: int) -> int:
    """hh_compress_blocks_bound: bytes that always hold n symbols compressed
    in blocks of block_syms with their own Huffman code."""
    return int(lib().hh_compress_blocks_bound(n, block_syms))


def encode_device(tree: "Tree", syms, out, stream=None) -> int:
    """Pack torch uint8 CUDA symbols with tree's codes into the torch uint8
    CUDA tensor out (hh_encode_device; out must hold the stream rounded up
    to 32-bit words, plus PAYLOAD_PAD for a decode).  Returns the bits."""
    import torch
    assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
    bits = C.c_uint64(0)
    _check(lib().hh_encode_device(C.byref(tree._c), syms.data_ptr(), syms.numel(), out.data_ptr(), out.numel(),
                                  C.byref(bits), stream.cuda_stream if stream is not None else None),
           "encode_device")
    return int(bits.value)


class Encoder:
    """A device encoder (hh_encoder_*): its own workspace, so that encoders
    on different streams (or threads) encode at once."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check(lib().hh_encoder_create(C.byref(self._h), device), "encoder create")

    def encode(self, tree: "Tree", syms, out, stream=None) -> int:
        """encode_device on this encoder."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        bits = C.c_uint64(0)
        _check(lib().hh_encoder_encode(self._h, C.byref(tree._c), syms.data_ptr(), syms.numel(), out.data_ptr(),
                                       out.numel(), C.byref(bits), stream.cuda_stream if stream is not None else None),
               "encoder_encode")
        return int(bits.value)

    def histogram(self, syms, stream=None) -> np.ndarray:
        """Exact byte counts (np.uint64[256]) of the torch uint8 CUDA tensor
        syms (hh_histogram_device; any alignment), on stream (default: the
        current one)."""
        import torch
        assert syms.is_cuda and syms.dtype == torch.uint8 and syms.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        counts = np.zeros(256, np.uint64)
        _check(lib().hh_histogram_device(self._h, syms.data_ptr() if syms.numel() else None, syms.numel(),
                                         counts.ctypes.data_as(C.POINTER(C.c_uint64)), s.cuda_stream), "histogram")
        return counts

    def compress(self, syms, out, stream=None) -> tuple:
        """Histogram, tree build and encode in one call (hh_compress_device):
        syms compressed into out (both torch uint8 CUDA tensors; out holds
        compress_bound(n) bytes, plus PAYLOAD_PAD for a decode) with their own
        Huffman code.  Returns (Tree, bits).  A HipHuffError of status -5
        (capacity) carries .tree and .bits."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        assert syms.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        tb = _TreeBuf()
        bits = C.c_uint64(0)
        rc = lib().hh_compress_device(self._h, syms.data_ptr() if syms.numel() else None, syms.numel(),
                                      out.data_ptr(), out.numel(), C.byref(tb), C.byref(bits), s.cuda_stream)
        if rc == -5:
            e = HipHuffError(rc, "compress")
            e.tree, e.bits = Tree._from_buf(tb), int(bits.value)
            raise e
        _check(rc, "compress")
        return Tree._from_buf(tb), int(bits.value)

    @staticmethod
    def _items_out_ptr(items_out, nb: int):
        """The device pointer of items_out, an int64 (nb, 4) CUDA tensor that
        receives the items for Decoder.decode_batch_items."""
        import torch
        if not (items_out.is_cuda and items_out.dtype == torch.int64 and items_out.is_contiguous()
                and tuple(items_out.shape) == (nb, 4)):
            raise ValueError(f"items_out: a contiguous CUDA int64 tensor of shape ({nb}, 4)")
        return items_out.data_ptr() if nb else None

    def encode_blocks(self, tree: "Tree", syms, block_syms: int, out, stream=None, items_out=None) -> tuple:
        """hh_encoder_encode_blocks: syms cut into blocks of block_syms, every
        block its own stream from the root, packed into out at 4-byte
        boundaries in one call (syms, out: torch uint8 CUDA tensors; out
        holds encode_blocks_bound(tree, n, block_syms) bytes, plus PAYLOAD_PAD
        for a decode).  Returns (items, total_bytes): items an (nb, 4) uint64
        array of (data_off, bits, out_off, cap) rows that goes straight into
        Decoder.decode_batch(out, items, dst).  A HipHuffError of status -5
        (capacity) carries .items and .total_bytes.  items_out: an int64
        (nb, 4) CUDA tensor that receives the same rows on the device
        (hh_encoder_encode_blocks_items), for Decoder.decode_batch_items."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        assert syms.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        n = syms.numel()
        items = np.zeros((_nblocks(n, block_syms), 4), np.uint64)
        total = C.c_uint64(0)
        if items_out is not None:
            rc = lib().hh_encoder_encode_blocks_items(self._h, C.byref(tree._c), syms.data_ptr() if n else None, n,
                                                      block_syms, out.data_ptr(), out.numel(),
                                                      self._items_out_ptr(items_out, items.shape[0]),
                                                      items.ctypes.data, C.byref(total), s.cuda_stream)
        else:
            rc = lib().hh_encoder_encode_blocks(self._h, C.byref(tree._c), syms.data_ptr() if n else None, n,
                                                block_syms, out.data_ptr(), out.numel(), items.ctypes.data,
                                                C.byref(total), s.cuda_stream)
        if rc == -5:
            e = HipHuffError(rc, "encoder_encode_blocks")
            e.items, e.total_bytes = items, int(total.value)
            raise e
        _check(rc, "encoder_encode_blocks")
        return items, int(total.value)

    def compress_blocks(self, syms, block_syms: int, out, stream=None, items_out=None) -> tuple:
        """hh_compress_blocks_device: histogram, one tree for all blocks, then
        encode_blocks with it (out holds compress_blocks_bound(n, block_syms)
        bytes, plus PAYLOAD_PAD for a decode).  Returns (Tree, items,
        total_bytes).  A HipHuffError of status -5 (capacity) carries .tree,
        .items and .total_bytes.  items_out: as in encode_blocks
        (hh_compress_blocks_device_items)."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        assert syms.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        n = syms.numel()
        tb = _TreeBuf()
        items = np.zeros((_nblocks(n, block_syms), 4), np.uint64)
        total = C.c_uint64(0)
        if items_out is not None:
            rc = lib().hh_compress_blocks_device_items(self._h, syms.data_ptr() if n else None, n, block_syms,
                                                       out.data_ptr(), out.numel(), C.byref(tb),
                                                       self._items_out_ptr(items_out, items.shape[0]),
                                                       items.ctypes.data, C.byref(total), s.cuda_stream)
        else:
            rc = lib().hh_compress_blocks_device(self._h, syms.data_ptr() if n else None, n, block_syms,
                                                 out.data_ptr(), out.numel(), C.byref(tb), items.ctypes.data,
                                                 C.byref(total), s.cuda_stream)
        if rc == -5:
            e = HipHuffError(rc, "compress_blocks")
            e.tree, e.items, e.total_bytes = Tree._from_buf(tb), items, int(total.value)
            raise e
        _check(rc, "compress_blocks")
        return Tree._from_buf(tb), items, int(total.value)

    @staticmethod
    def _ragged_offsets_dev(offsets, device, s):
        """offsets as a contiguous CUDA int64 (nrec + 1,) tensor; a host
        array is uploaded on the call's stream s."""
        import torch
        if not torch.is_tensor(offsets):
            h = _ragged_offsets(offsets).view(np.int64)
            with torch.cuda.stream(s):
                offsets = torch.from_numpy(h).to(device, non_blocking=True)
        if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.dim() == 1
                and offsets.numel() >= 1):
            raise ValueError("offsets: a contiguous CUDA int64 tensor of nrec + 1 values")
        return offsets

    def encode_ragged(self, tree: "Tree", syms, offsets, out, stream=None, items_out=None,
                      host_items: bool = True) -> tuple:
        """hh_encoder_encode_ragged: syms cut into records at offsets (a CUDA
        int64 (nrec + 1,) tensor: 0 first, nondecreasing, syms.numel() last; a
        host array is uploaded on the call's stream), every record its own
        stream from the root, packed into out at 4-byte boundaries in one
        call (syms, out: torch uint8 CUDA tensors; out holds
        encode_ragged_bound(tree, n, nrec) bytes, plus PAYLOAD_PAD for a
        decode).  Returns (items, total_bytes): items an (nrec, 4) uint64
        array of (data_off, bits, out_off, cap) rows for Decoder.decode_batch,
        or None with host_items=False (nothing per record crosses to the
        host).  items_out: an int64 (nrec, 4) CUDA tensor that receives the
        rows on the device, for Decoder.decode_batch_items.  A HipHuffError
        of status -5 (capacity) carries .items and .total_bytes."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        assert syms.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        offsets = self._ragged_offsets_dev(offsets, syms.device, s)
        n, nrec = syms.numel(), offsets.numel() - 1
        items = np.zeros((nrec, 4), np.uint64) if host_items else None
        total = C.c_uint64(0)
        rc = lib().hh_encoder_encode_ragged(
            self._h, C.byref(tree._c), syms.data_ptr() if n else None, n, offsets.data_ptr(), nrec, out.data_ptr(),
            out.numel(), self._items_out_ptr(items_out, nrec) if items_out is not None else None,
            items.ctypes.data if host_items and nrec else None, C.byref(total), s.cuda_stream)
        if rc == -5:
            e = HipHuffError(rc, "encoder_encode_ragged")
            e.items, e.total_bytes = items, int(total.value)
            raise e
        _check(rc, "encoder_encode_ragged")
        return items, int(total.value)

    def compress_ragged(self, syms, offsets, out, stream=None, items_out=None, host_items: bool = True) -> tuple:
        """hh_compress_ragged_device: histogram, one tree for all records,
        then encode_ragged with it (out holds compress_ragged_bound(n, nrec)
        bytes, plus PAYLOAD_PAD for a decode).  Returns (Tree, items,
        total_bytes).  A HipHuffError of status -5 (capacity) carries .tree,
        .items and .total_bytes."""
        import torch
        assert syms.is_cuda and out.is_cuda and syms.dtype == torch.uint8 and out.dtype == torch.uint8
        assert syms.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(syms.device)
        offsets = self._ragged_offsets_dev(offsets, syms.device, s)
        n, nrec = syms.numel(), offsets.numel() - 1
        tb = _TreeBuf()
        items = np.zeros((nrec, 4), np.uint64) if host_items else None
        total = C.c_uint64(0)
        rc = lib().hh_compress_ragged_device(
            self._h, syms.data_ptr() if n else None, n, offsets.data_ptr(), nrec, out.data_ptr(), out.numel(),
            C.byref(tb), self._items_out_ptr(items_out, nrec) if items_out is not None else None,
            items.ctypes.data if host_items and nrec else None, C.byref(total), s.cuda_stream)
        if rc == -5:
            e = HipHuffError(rc, "compress_ragged")
            e.tree, e.items, e.total_bytes = Tree._from_buf(tb), items, int(total.value)
            raise e
        _check(rc, "compress_ragged")
        return Tree._from_buf(tb), items, int(total.value)

    def close(self):
        if self._h:
            lib().hh_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compress_bound(n: int) -> int:
    """hh_compress_bound: bytes that always hold n symbols' stream."""
    return int(lib().hh_compress_bound(n))


def histogram_device(syms, stream=None) -> np.ndarray:
    """Encoder.histogram on a temporary encoder of syms' device."""
    enc = Encoder(syms.device.index or 0)
    try:
        return enc.histogram(syms, stream)
    finally:
        enc.close()


def compress_device(syms, stream=None) -> "HuffFile":
    """The torch uint8 CUDA tensor syms as a .huff container, compressed on
    the GPU with its own Huffman code (Encoder.compress); the payload is
    copied to the host."""
    import torch
    n = syms.numel()
    out = torch.zeros(compress_bound(n) + PAYLOAD_PAD, dtype=torch.uint8, device=syms.device)
    enc = Encoder(syms.device.index or 0)
    try:
        tree, bits = enc.compress(syms, out, stream)
    finally:
        enc.close()
    data = out[: (bits + 7) // 8 + PAYLOAD_PAD].cpu().numpy()
    data[(bits + 7) // 8:] = 0
    return HuffFile(tree.izero, tree.ione, tree.sym, bits, n, data)


def copy_device(src, dst, nt: bool = False, stream=None) -> float:
    """hh_copy_device on torch uint8 CUDA tensors (the same number of bytes,
    a multiple of 16): the streaming-copy reference; returns its device ms."""
    import torch
    assert src.is_cuda and dst.is_cuda and src.numel() == dst.numel()
    ms = C.c_float(0.0)
    s = stream if stream is not None else torch.cuda.current_stream(src.device)
    _check(lib().hh_copy_device(src.data_ptr(), dst.data_ptr(), src.numel(), int(nt), s.cuda_stream,
                                C.byref(ms)), "copy_device")
    return float(ms.value)


class RangeResult:
    """The hh_range_out of an asynchronous segment decode (valid once checked)."""

    def __init__(self):
        self._ro = _RangeOut()

    def as_dict(self) -> dict:
        ro = self._ro
        return {"out_len": int(ro.out_len), "leave_state": int(ro.leave_state),
                "const_seen": bool(ro.const_seen), "entry_state": int(ro.entry_state),
                "entry_exact": bool(ro.entry_exact)}


class Decoder:
    """Device decoder: tables + workspace on one GPU (hh_decoder_*)."""

    def __init__(self, device: int = 0, lane_bits: int = 0, flags: int = 0):
        self._h = C.c_void_p()
        cfg = _Config(device, lane_bits, flags)
        _check(lib().hh_decoder_create(C.byref(self._h), C.byref(cfg)), "decoder create")
        self.device = device
        self.flags = flags
        self._tree = None
        self._pending = []          # buffers of asynchronous decodes, kept alive until wait()
        self._pinned = None         # (payload, out) FLAG_KEEP_HOST_PINNED keeps registered
        self._batch_keep = None     # the tensors of the last decode_batch_items, which is not waited for

    def close(self):
        if self._h:
            lib().hh_decoder_destroy(self._h)   # (waits for an asynchronous decode or items batch still running)
            self._h = C.c_void_p()
        self._pending = []
        self._batch_keep = None
        self._pinned = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tree(self, tree: Tree):
        _check(lib().hh_decoder_set_tree(self._h, C.byref(tree._c)), "set tree")
        self._tree = tree

    def stats(self) -> dict:
        st = _Stats()
        _check(lib().hh_decoder_stats(self._h, C.byref(st)), "stats")
        return {k: getattr(st, k) for k, _ in _Stats._fields_}

    def decode_host(self, payload: np.ndarray, bits: int, cap: int,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
        """The evaluate() scope: host payload in, host symbols out.  `out`
        (uint8, >= cap) may be the caller's buffer, allocated and touched
        beforehand as evaluate() does (decodeUtil.c:37-38, 55)."""
        keep = bool(self.flags & FLAG_KEEP_HOST_PINNED)
        given = payload
        payload = np.ascontiguousarray(payload, np.uint8)
        # (copied: the caller's memory is not what gets registered -- a new
        # view of the same memory is fine, so the data pointers are compared)
        copied = not (isinstance(given, np.ndarray)
                      and given.__array_interface__["data"][0] == payload.__array_interface__["data"][0])
        if keep and (out is None or copied):
            # the decoder keeps both buffers registered after the call: they
            # must be the caller's own arrays, alive until release_host()
            # (a temporary freed after the call could be reallocated at the
            # same address and pass for the registered one)
            raise ValueError("FLAG_KEEP_HOST_PINNED: pass a contiguous uint8 payload and an `out` buffer")
        if out is None:
            out = np.zeros(max(cap, 1), np.uint8)
        assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size >= cap
        n = C.c_uint64(0)
        _check(lib().hh_decode_host(self._h, payload.ctypes.data, bits, out.ctypes.data, cap,
                                    C.byref(n)), "decode_host")
        if keep:
            self._pinned = (given, out)       # (alive while registered)
        return out[: n.value]

    def release_host(self) -> None:
        """hh_decoder_release_host: unpin the buffers FLAG_KEEP_HOST_PINNED kept."""
        _check(lib().hh_decoder_release_host(self._h), "release_host")
        self._pinned = None

    def decode_device_ptr(self, d_data: int, bits: int, d_out: int, cap: int,
                          stream: int = 0) -> int:
        n = C.c_uint64(0)
        _check(lib().hh_decode_device(self._h, d_data, bits, d_out, cap, C.byref(n),
                                      stream or None), "decode_device")
        return int(n.value)

    def decode_device(self, data, bits: int, out, stream=None) -> int:
        """Decode torch uint8 CUDA tensors (data holds payload + pad)."""
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8
        assert data.numel() >= (bits + 7) // 8 + PAYLOAD_PAD
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        return self.decode_device_ptr(data.data_ptr(), bits, out.data_ptr(), out.numel(),
                                      s.cuda_stream)

    def decode_device_async(self, data, bits: int, out, stream=None) -> "C.c_uint64":
        """hh_decode_device_async on torch tensors: enqueues the decode and
        returns a c_uint64 that holds its length once checked (by the next
        asynchronous decode or by wait()).  data, out and the returned
        object must live until wait() returns."""
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8
        assert data.numel() >= (bits + 7) // 8 + PAYLOAD_PAD
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        n = C.c_uint64(0)
        self._pending.append((data, out, n))
        _check(lib().hh_decode_device_async(self._h, data.data_ptr(), bits, out.data_ptr(), out.numel(),
                                            C.byref(n), s.cuda_stream), "decode_device_async")
        return n

    def wait(self) -> None:
        """hh_decode_wait: every asynchronous decode checked; raises the first
        failure among them."""
        rc = lib().hh_decode_wait(self._h)
        self._pending = []
        _check(rc, "decode_wait")

    def decode_batch(self, data, items, out, stream=None) -> tuple:
        """hh_decode_batch_device: n independent streams of this decoder's
        code in one launch.  data, out: torch uint8 CUDA tensors; items: an
        (n, 4) uint64 array of (data_off, bits, out_off, cap) rows, the
        fields of hh_batch_item.  Returns (out_len np.uint64[n], status
        np.int32[n]).  A failing batch raises HipHuffError with the status
        of its lowest-index failing stream (.status, as every HipHuffError),
        carrying the two arrays as .out_len and .statuses."""
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8 and out.dtype == torch.uint8
        assert data.is_contiguous() and out.is_contiguous()
        items = np.ascontiguousarray(items, np.uint64)
        if items.ndim != 2 or items.shape[1] != 4:
            raise ValueError("items: an (n, 4) array of (data_off, bits, out_off, cap)")
        n = items.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        out_len = np.zeros(n, np.uint64)
        status = np.zeros(n, np.int32)
        rc = lib().hh_decode_batch_device(self._h, data.data_ptr(), data.numel(), items.ctypes.data, n,
                                          out.data_ptr(), out.numel(),
                                          out_len.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          status.ctypes.data_as(C.POINTER(C.c_int32)), s.cuda_stream)
        if rc != 0:
            e = HipHuffError(rc, "decode_batch")
            e.out_len, e.statuses = out_len, status
            raise e
        return out_len, status

    def decode_batch_items(self, data, items, out, out_len=None, status=None, summary=False, stream=None,
                           data_bytes: Optional[int] = None, out_bytes: Optional[int] = None) -> tuple:
        """hh_decode_batch_device_items: decode_batch with the items, the
        lengths and the statuses on the device, enqueued on stream (default:
        the current one) without synchronising.  items: a CUDA int64 (n, 4)
        tensor of (data_off, bits, out_off, cap) rows (values below 2^63);
        out_len (int64, n) and status (int32, n): CUDA tensors, allocated
        when not given (in the stream's pool).  Returns (out_len, status),
        with summary=True or summary=<an int32[6] CUDA tensor> (out_len,
        status, summary): the tensor holds hh_batch_summary
        (batch_summary() reads it).  All of them are
        complete once the stream has passed the call's work.  An item that
        breaks a rule gets status -1 and length 0 and the others decode;
        only what the host can check raises.  data_bytes / out_bytes: the
        sizes the items are checked against (default: the tensors').  The
        tensors are kept alive until the next batch call on this decoder or
        close()."""
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8 and out.dtype == torch.uint8
        assert data.is_contiguous() and out.is_contiguous()
        if not (items.is_cuda and items.dtype == torch.int64 and items.is_contiguous() and items.dim() == 2
                and items.shape[1] == 4):
            raise ValueError("items: a contiguous CUDA int64 tensor of (data_off, bits, out_off, cap) rows")
        n = items.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        with torch.cuda.stream(s):
            if out_len is None:
                out_len = torch.empty(n, dtype=torch.int64, device=data.device)
            if status is None:
                status = torch.empty(n, dtype=torch.int32, device=data.device)
            if summary is True:
                summ = torch.empty(6, dtype=torch.int32, device=data.device)
            else:
                summ = None if summary is False or summary is None else summary
        assert summ is None or (summ.is_cuda and summ.dtype == torch.int32 and summ.is_contiguous()
                                and summ.numel() == 6)
        assert out_len.is_cuda and out_len.dtype == torch.int64 and out_len.is_contiguous() and out_len.numel() == n
        assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == n
        self._batch_keep = (data, items, out, out_len, status, summ)
        rc = lib().hh_decode_batch_device_items(
            self._h, data.data_ptr(), data.numel() if data_bytes is None else data_bytes,
            items.data_ptr() if n else None, n, out.data_ptr(), out.numel() if out_bytes is None else out_bytes,
            out_len.data_ptr() if n else None, status.data_ptr() if n else None,
            summ.data_ptr() if summ is not None else None, s.cuda_stream)
        _check(rc, "decode_batch_items")
        return (out_len, status, summ) if summ is not None else (out_len, status)

    def read_blocks(self, data, index, n_syms: int, block_syms: int, reads, out, read_len=None, status=None,
                    summary=False, stream=None, data_bytes: Optional[int] = None,
                    out_bytes: Optional[int] = None) -> tuple:
        """hh_decode_blocks_read: byte ranges of the uncompressed data of a
        block-coded buffer, each delivered to its own place in out, enqueued
        on stream (default: the current one) without synchronising.  data:
        the blocks' payload; index: the CUDA int64 (nb, 4) tensor that
        Encoder.encode_blocks(..., items_out=t) fills, for n_syms symbols in
        blocks of block_syms; reads: a CUDA int64 (m, 3) tensor of (src_off,
        len, dst_off) rows (a host array of that shape is uploaded on the
        call's stream).  read_len (int64, m), status (int32, m) and summary
        as in decode_batch_items.  Returns (read_len, status[, summary]),
        complete once the stream has passed the call's work.  A read that
        breaks a rule gets status -1, one whose block ends early -3
        (read_len the bytes delivered), and the others are served; only what
        the host can check raises.  The tensors are kept alive until the
        next batch call on this decoder or close()."""
        return self._blocks_call("hh_decode_blocks_read", "read_blocks", data, index, n_syms, block_syms, reads, out,
                                 read_len, status, summary, stream, data_bytes, out_bytes)

    def gather_blocks(self, data, index, n_syms: int, block_syms: int, reads, out, read_len=None, status=None,
                      summary=False, stream=None, data_bytes: Optional[int] = None,
                      out_bytes: Optional[int] = None) -> tuple:
        """hh_decode_blocks_gather: read_blocks with every touched block
        walked once per call for all the reads that fall into it -- the call
        for dense small reads (several per block).  Parameters, results,
        statuses and stream order are read_blocks'; the number of blocks must
        be below 2^32 - 1 (the call keeps a few words per block and scans
        them on every call)."""
        return self._blocks_call("hh_decode_blocks_gather", "gather_blocks", data, index, n_syms, block_syms, reads,
                                 out, read_len, status, summary, stream, data_bytes, out_bytes)

    def _blocks_call(self, fn, what, data, index, n_syms, block_syms, reads, out, read_len, status, summary, stream,
                     data_bytes, out_bytes) -> tuple:
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8 and out.dtype == torch.uint8
        assert data.is_contiguous() and out.is_contiguous()
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        if not torch.is_tensor(reads):
            h = np.ascontiguousarray(reads)
            if h.ndim != 2 or h.shape[1] != 3:
                raise ValueError("reads: an (m, 3) array of (src_off, len, dst_off)")
            h = h.astype(np.uint64, copy=False).view(np.int64)
            with torch.cuda.stream(s):
                reads = torch.from_numpy(h).to(data.device, non_blocking=True)
        if not (reads.is_cuda and reads.dtype == torch.int64 and reads.is_contiguous() and reads.dim() == 2
                and reads.shape[1] == 3):
            raise ValueError("reads: a contiguous CUDA int64 tensor of (src_off, len, dst_off) rows")
        nb = _nblocks(n_syms, block_syms) if block_syms > 0 else index.shape[0]
        if not (index.is_cuda and index.dtype == torch.int64 and index.is_contiguous()
                and tuple(index.shape) == (nb, 4)):
            raise ValueError(f"index: a contiguous CUDA int64 tensor of shape ({nb}, 4)")
        m = reads.shape[0]
        with torch.cuda.stream(s):
            if read_len is None:
                read_len = torch.empty(m, dtype=torch.int64, device=data.device)
            if status is None:
                status = torch.empty(m, dtype=torch.int32, device=data.device)
            if summary is True:
                summ = torch.empty(6, dtype=torch.int32, device=data.device)
            else:
                summ = None if summary is False or summary is None else summary
        assert summ is None or (summ.is_cuda and summ.dtype == torch.int32 and summ.is_contiguous()
                                and summ.numel() == 6)
        assert read_len.is_cuda and read_len.dtype == torch.int64 and read_len.is_contiguous() and read_len.numel() == m
        assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == m
        self._batch_keep = (data, index, reads, out, read_len, status, summ)
        rc = getattr(lib(), fn)(
            self._h, data.data_ptr(), data.numel() if data_bytes is None else data_bytes,
            index.data_ptr() if nb else None, n_syms, block_syms, reads.data_ptr() if m else None, m,
            out.data_ptr(), out.numel() if out_bytes is None else out_bytes,
            read_len.data_ptr() if m else None, status.data_ptr() if m else None,
            summ.data_ptr() if summ is not None else None, s.cuda_stream)
        _check(rc, what)
        return (read_len, status, summ) if summ is not None else (read_len, status)

    def take_records(self, data, index, ids, out, out_offs=None, status=None, summary=False, stream=None,
                     data_bytes: Optional[int] = None, out_bytes: Optional[int] = None) -> tuple:
        """hh_decode_batch_take: the records of a coded column named by ids,
        their bytes one after another in out and the offsets that delimit
        them, enqueued on stream (default: the current one) without
        synchronising.  data: the records' payload; index: the CUDA int64
        (nrec, 4) tensor Encoder.encode_ragged(..., items_out=t) (or
        encode_blocks) fills; ids: a CUDA int64 tensor of m record ids
        (uint64 values viewed as int64; a host array is uploaded on the
        call's stream), None: all records in order.  out_offs (int64, m + 1),
        status (int32, m) and summary as in decode_batch_items.  Returns
        (out_offs, status[, summary]), complete once the stream has passed
        the call's work.  A bad id or index row gets status -1 and length 0,
        a record past out's end -2, one whose stream and length disagree -3,
        and the others decode; only what the host can check raises.  The
        tensors are kept alive until the next batch call on this decoder or
        close()."""
        import torch
        assert data.is_cuda and out.is_cuda and data.dtype == torch.uint8 and out.dtype == torch.uint8
        assert data.is_contiguous() and out.is_contiguous()
        if not (index.is_cuda and index.dtype == torch.int64 and index.is_contiguous() and index.dim() == 2
                and index.shape[1] == 4):
            raise ValueError("index: a contiguous CUDA int64 tensor of (data_off, bits, out_off, cap) rows")
        nrec = index.shape[0]
        s = stream if stream is not None else torch.cuda.current_stream(data.device)
        if ids is not None and not torch.is_tensor(ids):
            h = np.ascontiguousarray(ids).astype(np.uint64, copy=False).view(np.int64).reshape(-1)
            with torch.cuda.stream(s):
                ids = torch.from_numpy(h).to(data.device, non_blocking=True)
        if ids is not None and not (ids.is_cuda and ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 1):
            raise ValueError("ids: a contiguous CUDA int64 tensor of record ids, or None")
        m = nrec if ids is None else ids.shape[0]
        with torch.cuda.stream(s):
            if out_offs is None:
                out_offs = torch.empty(m + 1, dtype=torch.int64, device=data.device)
            if status is None:
                status = torch.empty(m, dtype=torch.int32, device=data.device)
            if summary is True:
                summ = torch.empty(6, dtype=torch.int32, device=data.device)
            else:
                summ = None if summary is False or summary is None else summary
        assert summ is None or (summ.is_cuda and summ.dtype == torch.int32 and summ.is_contiguous()
                                and summ.numel() == 6)
        assert out_offs.is_cuda and out_offs.dtype == torch.int64 and out_offs.is_contiguous() \
            and out_offs.numel() == m + 1
        assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() == m
        self._batch_keep = (data, index, ids, out, out_offs, status, summ)
        rc = lib().hh_decode_batch_take(
            self._h, data.data_ptr(), data.numel() if data_bytes is None else data_bytes,
            # (an empty list of ids reads no index: nrec 0 beside the NULL of an empty tensor)
            index.data_ptr() if nrec and m else None, nrec if m else 0, ids.data_ptr() if ids is not None and m else None, m,
            out.data_ptr(), out.numel() if out_bytes is None else out_bytes,
            out_offs.data_ptr() if m else None, status.data_ptr() if m else None,
            summ.data_ptr() if summ is not None else None, s.cuda_stream)
        _check(rc, "take_records")
        return (out_offs, status, summ) if summ is not None else (out_offs, status)

    def take_round_tiles(self) -> int:
        """hh_decode_take_round_tiles: tiles per round of take_records'
        kernel for the current tree (a round holds 64 x tiles regions of
        geometry()["S"] bits, of as many records as fall into them)."""
        w = C.c_uint32(0)
        _check(lib().hh_decode_take_round_tiles(self._h, C.byref(w)), "take_round_tiles")
        return int(w.value)

    @staticmethod
    def batch_summary(summary) -> dict:
        """The hh_batch_summary in decode_batch_items' or read_blocks' summary tensor
        (a copy to the host on the current stream: synchronise the batch's
        stream first when it is another one)."""
        w = summary.cpu().numpy().view(np.uint32)
        return {"total_len": int(w[0]) | int(w[1]) << 32, "n_failed": int(w[2]), "first_failed": int(w[3]),
                "first_status": int(w[4:5].view(np.int32)[0])}

    def batch_round_tiles(self) -> int:
        """hh_decode_batch_round_tiles: tiles per round of a workgroup of the
        batched decode, for the current tree."""
        w = C.c_uint32(0)
        _check(lib().hh_decode_batch_round_tiles(self._h, C.byref(w)), "batch_round_tiles")
        return int(w.value)

    def geometry(self) -> dict:
        """hh_debug_geometry: what set_tree chose for the batched decode --
        region bits S, emission step K, remainder step r, count step bits cb,
        the batch's head G, its tiles per round W, the states ns and
        k_batch's LDS bytes."""
        g = (C.c_uint32 * 8)()
        _check(lib().hh_debug_geometry(self._h, g), "geometry")
        return dict(zip(("S", "K", "r", "cb", "G", "W", "ns", "lds"), (int(v) for v in g)))

    def tile_bits(self) -> int:
        """Bits per tile for the current tree (segments are whole tiles)."""
        tb = C.c_uint64(0)
        _check(lib().hh_decoder_tile_bits(self._h, C.byref(tb)), "tile_bits")
        return int(tb.value)

    def decode_range_ptr(self, d_data: int, bits_avail: int, ntiles: int, in_state: int,
                         d_out: int, cap: int, stream: int = 0, prologue: int = 0) -> dict:
        """One segment (hh_decode_device_range): tiles [0, ntiles) of the
        bits at d_data, entered in state in_state; the first `prologue`
        tiles only locate the entry of tile `prologue`."""
        rg = _Range(bits_avail, ntiles, prologue, in_state)
        ro = _RangeOut()
        _check(lib().hh_decode_device_range(self._h, d_data, C.byref(rg), d_out, cap,
                                            C.byref(ro), stream or None), "decode_range")
        return {"out_len": int(ro.out_len), "leave_state": int(ro.leave_state),
                "const_seen": bool(ro.const_seen), "entry_state": int(ro.entry_state),
                "entry_exact": bool(ro.entry_exact)}

    def decode_range_async_ptr(self, d_data: int, bits_avail: int, ntiles: int, in_state: int,
                               d_out: int, cap: int, stream: int = 0, prologue: int = 0) -> "RangeResult":
        """hh_decode_device_range_async: enqueues the segment's decode and
        returns a RangeResult whose fields are valid once the decode has been
        checked (by the next asynchronous decode on this decoder, or wait())."""
        rg = _Range(bits_avail, ntiles, prologue, in_state)
        r = RangeResult()
        self._pending.append(r)
        _check(lib().hh_decode_device_range_async(self._h, d_data, C.byref(rg), d_out, cap,
                                                  C.byref(r._ro), stream or None), "decode_range_async")
        return r

    def stage_pipeline_ptr(self, d_data: int, bits: int, d_out: int, cap: int,
                           stream: int = 0) -> int:
        n = C.c_uint64(0)
        _check(lib().hh_stage_pipeline(self._h, d_data, bits, d_out, cap, C.byref(n),
                                       stream or None), "stage_pipeline")
        return int(n.value)


def decode_file(path: str, device: int = 0) -> np.ndarray:
    """Load a .huff and decode it on the GPU (host-to-host)."""
    hf = HuffFile.load(path)
    dec = Decoder(device)
    try:
        dec.set_tree(hf.tree())
        return dec.decode_host(hf.payload, hf.bits, hf.bits + 1)
    finally:
        dec.close()
