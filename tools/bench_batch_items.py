"""Batched decode from a device item list against the host-items call, by the
protocol of tools/bench_batch.py: kjv.txt tiled, every block encoded on its
own with one shared code, everything resident in HBM.  Per shape

  (a)      a_ms       one hh_decode_batch_device call (host items; returns when done);
  (d)      d_ms       one hh_decode_batch_device_items call, to the end event on the stream;
  (d-host) d_host_ms  the host's wall time inside the (d) call alone, no sync.

(a) and (d) alternate in one process; a figure is the median of --reps runs
after --warmup, device events around the call; the whole series is repeated
--series times and the medians' range is the spread.  Both outputs are
compared byte for byte before anything is timed.  The shape "mixed" is the
lengths of tests/test_gpu_batch_items.py's mixed batch scaled to about 64 MiB
of text (empty, tiny, half a round to three rounds, one past the plan's
clamp).

    python tools/bench_batch_items.py [--reps 20] [--warmup 3] [--series 3] [--only a|d]
        [--shapes 64:1024,4:16384,1024:64,mixed] [--out profiles/batch_items_bench.json]

--only a / --only d runs one path alone (for a kernel trace of its own:
rocprofv3 --kernel-trace --stats -- python tools/bench_batch_items.py --only d).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import huffmandecoderongpus_amd as H  # noqa: E402
from huffmandecoderongpus_amd import synth  # noqa: E402


def block_lengths(spec, dec, kjv_size):
    """The blocks' text lengths of a shape."""
    if spec != "mixed":
        kib, nblk = (int(x) for x in spec.split(":"))
        return [kib << 10] * nblk
    # a round's text, about: its bits over kjv's bits per symbol
    rb = 64 * dec.batch_round_tiles() * (dec.tile_bits() // 64)
    per = rb / 8 * 1.75
    rng = np.random.default_rng(600)
    lens = [0] * 5 + [int(v) for v in rng.integers(1, 200, 400)]
    lens += [int(per * (0.5 + 2.5 * k / 190)) for k in range(190)] * 5
    lens += [int(per * 64)]
    return [lens[i] for i in rng.permutation(len(lens))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--only", choices=["a", "d"], default=None)
    ap.add_argument("--shapes", default="64:1024,4:16384,1024:64,mixed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_items: needs a GPU")
    tree = H.HuffFile.load(os.path.join(ROOT, "files", "kjv.txt.huff")).tree()
    kjv = synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1]
    dec = H.Decoder(0)
    dec.set_tree(tree)
    rows = []
    for spec in a.shapes.split(","):
        lens = block_lengths(spec, dec, kjv.size)
        n, nblk = sum(lens), len(lens)
        text = np.tile(kjv, n // kjv.size + 1)[:n]
        starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        enc = [tree.encode(text[starts[i]: starts[i + 1]]) if lens[i] else (np.zeros(0, np.uint8), 0)
               for i in range(nblk)]
        offs, at = [], 0
        for p, b in enc:
            offs.append(at)
            at += ((b + 7) // 8 + 3) // 4 * 4
        data = np.zeros(at + H.PAYLOAD_PAD, np.uint8)
        for (p, b), o in zip(enc, offs):
            data[o: o + (b + 7) // 8] = p[: (b + 7) // 8]
        items = np.array([[o, b, int(starts[i]), lens[i]] for i, ((_, b), o) in enumerate(zip(enc, offs))],
                         np.uint64).reshape(-1, 4)
        d_data = torch.from_numpy(data).cuda()
        d_items = torch.from_numpy(items.view(np.int64)).cuda()
        want = torch.from_numpy(text).cuda()
        out_a = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        out_d = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(nblk, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(nblk, dtype=torch.int32, device="cuda")
        d_sum = torch.zeros(6, dtype=torch.int32, device="cuda")
        host = []

        def fa():
            dec.decode_batch(d_data, items, out_a)

        def fd():
            t0 = time.perf_counter()
            dec.decode_batch_items(d_data, d_items, out_d, d_len, d_st, d_sum)
            host.append((time.perf_counter() - t0) * 1e3)

        # one checked run of each
        len_a, _ = dec.decode_batch(d_data, items, out_a)
        fd()
        torch.cuda.synchronize()
        summ = dec.batch_summary(d_sum)
        ok = (bool((len_a == items[:, 3]).all()) and torch.equal(out_a[:n], want) and torch.equal(out_d[:n], want)
              and np.array_equal(d_len.cpu().numpy().astype(np.uint64), len_a) and not d_st.any().item()
              and summ["n_failed"] == 0 and summ["total_len"] == n)
        paths = [p for p in (("a", fa), ("d", fd)) if a.only in (None, p[0])]
        med = {k: [] for k, _ in paths}
        med_host = []
        for _ in range(a.series):
            ms = {k: [] for k, _ in paths}
            host.clear()
            for i in range(a.warmup + a.reps):
                for k, fn in paths:                              # (alternating)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        ms[k].append(e0.elapsed_time(e1))
            for k in ms:
                med[k].append(statistics.median(ms[k]))
            if host:
                med_host.append(statistics.median(host[a.warmup:]))
        row = {"shape": spec, "blocks": nblk, "text_mib": round(n / 2 ** 20, 2), "ok": ok,
               "round_tiles": dec.batch_round_tiles()}
        for k in med:
            row[k + "_ms"] = round(statistics.median(med[k]), 4)
            row[k + "_series"] = [round(v, 4) for v in med[k]]
            row[k + "_spread_ms"] = round(max(med[k]) - min(med[k]), 4)
        if med_host:
            row["d_host_ms"] = round(statistics.median(med_host), 4)
        if "a" in med and "d" in med:
            row["d_minus_a_ms"] = round(row["d_ms"] - row["a_ms"], 4)
            row["d_within_a_spread"] = row["d_ms"] <= row["a_ms"] + row["a_spread_ms"]
        rows.append(row)
        del d_data, want, out_a, out_d
        torch.cuda.empty_cache()
    dec.close()
    res = {"bench": "batch_items", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "series": a.series, "only": a.only,
           "protocol": "median of reps after warmup, device events around each call, (a) and (d) alternating; "
                       "spread: range of the series' medians", "rows": rows}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
