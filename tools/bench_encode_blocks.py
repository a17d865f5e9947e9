"""Blocked-encode timing: one text cut into blocks, every block encoded as
its own stream with one shared code, everything resident in HBM.  For every
shape it times

  (a) blocks_ms  one hh_encoder_encode_blocks call for all blocks;
  (b) loop_ms    the same blocks as a loop of hh_encoder_encode, one call per
                 block, into the 4-byte-aligned offsets of one buffer (what a
                 user had before the blocked call);
  (c) single_ms  one hh_encoder_encode of the whole text as a single stream:
                 the floor (the same passes without the block scan, the
                 per-block read-back and the item list).

Prints one JSON line (and writes it to --out).

    python tools/bench_encode_blocks.py [--reps 20] [--warmup 3] [--out profiles/encode_blocks_bench.json]
                                        [--shapes 64:1024,4:16384,1024:64]

A shape is KiB-of-text-per-block:blocks; the text is kjv.txt tiled.  Every
figure is the median of --reps runs after --warmup, timed with device events
around the call(s) on the current stream; all three return to the host inside
that window (the encoder's calls are synchronous).  Before anything is timed,
(a)'s buffer is compared byte for byte with (b)'s, and hh_decode_batch_device
of (a)'s buffer with (a)'s items must give the text back.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import huffmandecoderongpus_amd as H  # noqa: E402
from huffmandecoderongpus_amd import synth  # noqa: E402


def timed(fn, reps, warmup):
    """Median device ms of fn() (events on the current stream)."""
    ms = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="64:1024,4:16384,1024:64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_encode_blocks: needs a GPU")
    hf = H.HuffFile.load(os.path.join(ROOT, "files", "kjv.txt.huff"))
    tree = hf.tree()
    kjv = synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1]
    enc = H.Encoder(0)
    dec = H.Decoder(0)
    dec.set_tree(tree)
    L = H.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for spec in a.shapes.split(","):
        kib, nblk = (int(x) for x in spec.split(":"))
        blk = kib << 10
        n = blk * nblk
        d_text = torch.from_numpy(np.tile(kjv, n // kjv.size + 1)[:n]).cuda()
        cap = H.encode_blocks_bound(tree, n, blk)
        out_a = torch.full((cap + H.PAYLOAD_PAD,), 0xAB, dtype=torch.uint8, device="cuda")
        out_b = torch.zeros(cap + H.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
        out_c = torch.zeros(cap + H.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
        back = torch.zeros(n, dtype=torch.uint8, device="cuda")
        bits = C.c_uint64(0)

        def blocks():
            return enc.encode_blocks(tree, d_text, blk, out_a[:cap])

        # one checked run of (a): it gives (b) its offsets
        items, total = blocks()
        offs = [int(o) for o in items[:, 0]]

        def loop():
            for i in range(nblk):
                rc = L.hh_encoder_encode(enc._h, C.byref(tree._c), d_text.data_ptr() + i * blk, blk,
                                         out_b.data_ptr() + offs[i], cap - offs[i], C.byref(bits), stream)
                if rc:
                    raise H.HipHuffError(rc, "encoder_encode")

        def single():
            return enc.encode(tree, d_text, out_c[:cap])

        loop()
        ok = torch.equal(out_a[:total], out_b[:total]) and int(out_a[total:].ne(0xAB).sum()) == 0
        out_len, status = dec.decode_batch(out_a[: total + H.PAYLOAD_PAD], items, back)
        ok = ok and not status.any() and bool((out_len == blk).all()) and torch.equal(back, d_text)
        wbits = single()
        ok = ok and wbits == int(items[:, 1].sum())
        single_ms = timed(single, a.reps, a.warmup)
        blocks_ms = timed(blocks, a.reps, a.warmup)
        loop_ms = timed(loop, a.reps, a.warmup)
        rows.append({
            "block_kib": kib, "blocks": nblk, "text_mib": n >> 20, "ok": bool(ok),
            "total_bytes": total, "single_bytes": (wbits + 31) // 32 * 4,
            "blocks_ms": round(blocks_ms, 4), "loop_ms": round(loop_ms, 4), "single_ms": round(single_ms, 4),
            "loop_over_blocks": round(loop_ms / blocks_ms, 2), "blocks_over_single": round(blocks_ms / single_ms, 2),
            "blocks_gbs_in": round(n / blocks_ms * 1e-6, 1),
        })
        del d_text, out_a, out_b, out_c, back
        torch.cuda.empty_cache()
    dec.close()
    enc.close()
    res = {"bench": "encode_blocks", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "protocol": "median, device events around each call", "rows": rows}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
