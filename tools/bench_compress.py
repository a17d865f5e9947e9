"""Compression timing: Encoder.histogram and Encoder.compress with the input
resident in HBM, beside two yardsticks taken on the same tensor in the same
process -- torch.bincount(syms, minlength=256) (what a user has without this
library) and the read rate of hh_copy_device (what a pure streaming pass
reaches).  Prints one JSON line (and writes it to --out).

    python tools/bench_compress.py [--reps 20] [--warmup 3] [--out profiles/compress_bench.json]
                                   [--inputs kjv:64,kjv:256,kjv:1024,zipf:256]

Inputs: kjv.txt tiled to the MiB given; synth.byte_stream's Zipf bytes (the
low-skew case).  Every figure is the median of --reps runs after --warmup,
timed with device events around the call on the current stream; histogram,
bincount and compress return to the host inside that window (each ends in a
read-back), so their times include that wait -- the pure kernel times of the
histogram are tools/ubench/ub_hist.hip's.  compress_ms - (hist_ms +
encode_ms) is compress's host gap: the tree build and one more sync.
"""
import argparse
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
    ap.add_argument("--inputs", default="kjv:64,kjv:256,kjv:1024,zipf:256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_compress: needs a GPU")
    kjv = None
    enc = H.Encoder(0)
    rows = []
    for spec in a.inputs.split(","):
        kind, mib = spec.split(":")
        n = int(mib) << 20
        if kind == "kjv":
            if kjv is None:
                kjv = torch.from_numpy(synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1].copy()).cuda()
            syms = kjv.repeat(n // kjv.numel() + 1)[:n].contiguous()
        elif kind == "zipf":
            syms = synth.byte_stream(n).syms[:n].contiguous()   # (more symbols than payload bytes)
            assert syms.numel() == n
        else:
            raise SystemExit(f"unknown input {spec}")
        dst = torch.empty_like(syms)
        out = torch.zeros(H.compress_bound(n) + H.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
        # one checked run of each
        counts = enc.histogram(syms)
        ref = torch.bincount(syms, minlength=256).cpu().numpy().astype(np.uint64)
        ok = bool(np.array_equal(counts, ref))
        tree, bits = enc.compress(syms, out)
        ok = ok and enc.encode(tree, syms, out) == bits
        copy_ms = statistics.median([H.copy_device(syms, dst, nt=True) for _ in range(a.warmup + a.reps)][a.warmup:])
        binc_ms = timed(lambda: torch.bincount(syms, minlength=256), a.reps, a.warmup)
        hist_ms = timed(lambda: enc.histogram(syms), a.reps, a.warmup)
        enc_ms = timed(lambda: enc.encode(tree, syms, out), a.reps, a.warmup)
        comp_ms = timed(lambda: enc.compress(syms, out), a.reps, a.warmup)
        gbs = lambda ms: n / ms * 1e-6   # noqa: E731
        rows.append({
            "input": kind, "mib": int(mib), "ok": ok, "bits_per_symbol": round(bits / n, 4),
            "copy_ms": round(copy_ms, 4), "copy_read_gbs": round(gbs(copy_ms), 1),
            "bincount_ms": round(binc_ms, 4),
            "hist_ms": round(hist_ms, 4), "hist_gbs": round(gbs(hist_ms), 1),
            "hist_frac_of_copy": round(copy_ms / hist_ms, 3), "bincount_over_hist": round(binc_ms / hist_ms, 2),
            "encode_ms": round(enc_ms, 4), "compress_ms": round(comp_ms, 4),
            "compress_host_gap_ms": round(comp_ms - hist_ms - enc_ms, 4),
        })
        del syms, dst, out
        torch.cuda.empty_cache()
    enc.close()
    res = {"bench": "compress", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
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
