"""Batched-decode timing: many blocks of one text, each encoded on its own
with one shared code, everything resident in HBM.  For every shape it times

  (a) batch_ms   one hh_decode_batch_device call for all blocks;
  (b) loop_ms    the same blocks as a loop of hh_decode_device_async plus one
                 hh_decode_wait on one decoder (what a user had before the
                 batch call);
  (c) single_ms  one hh_decode_device of the same text encoded as a single
                 stream: the ceiling.

Prints one JSON line (and writes it to --out).

    python tools/bench_batch.py [--reps 20] [--warmup 3] [--out profiles/batch_bench.json]
                                [--shapes 64:1024,4:16384,1024:64]

A shape is KiB-of-text-per-block:blocks; the text is kjv.txt tiled.  Every
figure is the median of --reps runs after --warmup, timed with device events
around the call(s) on the current stream; (a) and (b) return to the host
inside that window, so their times include the descriptor upload, the result
read-back and the host's share of the launches.  batch_kernel_ms is the
launch's own device time (hh_stats.ms_total).  All three outputs are compared
byte for byte before anything is timed.
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
        raise SystemExit("bench_batch: needs a GPU")
    hf = H.HuffFile.load(os.path.join(ROOT, "files", "kjv.txt.huff"))
    tree = hf.tree()
    kjv = synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1]
    dec = H.Decoder(0)
    dec.set_tree(tree)
    L = H.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for spec in a.shapes.split(","):
        kib, nblk = (int(x) for x in spec.split(":"))
        blk = kib << 10
        n = blk * nblk
        text = np.tile(kjv, n // kjv.size + 1)[:n]
        # the blocks, each encoded on its own, packed at 4-byte boundaries
        enc = [tree.encode(text[i * blk: (i + 1) * blk]) for i in range(nblk)]
        offs, at = [], 0
        for p, b in enc:
            offs.append(at)
            at += ((b + 7) // 8 + 3) // 4 * 4
        data = np.zeros(at + H.PAYLOAD_PAD, np.uint8)
        for (p, b), o in zip(enc, offs):
            data[o: o + (b + 7) // 8] = p[: (b + 7) // 8]
        items = np.array([[o, b, i * blk, blk] for i, ((_, b), o) in enumerate(zip(enc, offs))], np.uint64)
        d_data = torch.from_numpy(data).cuda()
        whole, wbits = tree.encode(text)
        d_whole = torch.from_numpy(whole).cuda()
        out_c = torch.zeros(n, dtype=torch.uint8, device="cuda")
        out_a = torch.zeros(n, dtype=torch.uint8, device="cuda")
        out_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
        lens = np.zeros(nblk, np.uint64)
        plen = [C.cast(lens.ctypes.data + 8 * i, C.POINTER(C.c_uint64)) for i in range(nblk)]

        def batch():
            return dec.decode_batch(d_data, items, out_a)

        def loop():
            for i in range(nblk):
                rc = L.hh_decode_device_async(dec._h, d_data.data_ptr() + offs[i], int(items[i, 1]),
                                              out_b.data_ptr() + i * blk, blk,
                                              plen[i], stream)
                if rc:
                    raise H.HipHuffError(rc, "decode_device_async")
            rc = L.hh_decode_wait(dec._h)
            if rc:
                raise H.HipHuffError(rc, "decode_wait")

        def single():
            return dec.decode_device(d_whole, wbits, out_c)

        # one checked run of each
        ok = single() == n and bool((out_c.cpu().numpy() == text).all())
        out_len, _ = batch()
        ok = ok and bool((out_len == blk).all()) and torch.equal(out_a, out_c)
        loop()
        ok = ok and bool((lens == blk).all()) and torch.equal(out_b, out_c)
        single_ms = timed(single, a.reps, a.warmup)
        kern = []

        def batch_k():
            batch()
            kern.append(dec.stats()["ms_total"])

        batch_ms = timed(batch_k, a.reps, a.warmup)
        loop_ms = timed(loop, a.reps, a.warmup)
        rows.append({
            "block_kib": kib, "blocks": nblk, "text_mib": n >> 20, "ok": ok,
            "round_tiles": dec.batch_round_tiles(),
            "batch_ms": round(batch_ms, 4), "batch_kernel_ms": round(statistics.median(kern[a.warmup:]), 4),
            "loop_ms": round(loop_ms, 4), "single_ms": round(single_ms, 4),
            "loop_over_batch": round(loop_ms / batch_ms, 2), "batch_over_single": round(batch_ms / single_ms, 2),
            "batch_gbs_out": round(n / batch_ms * 1e-6, 1),
        })
        del d_data, d_whole, out_a, out_b, out_c
        torch.cuda.empty_cache()
    dec.close()
    res = {"bench": "batch", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
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
