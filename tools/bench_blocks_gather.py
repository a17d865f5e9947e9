"""Gathered range reads (hh_decode_blocks_gather) beside the two older ways to
serve reads from a block-coded buffer, by the protocol of
tools/bench_blocks_read.py: kjv.txt tiled to --mib MiB in blocks of
--block-kib KiB under one shared code, everything resident in HBM.  Shapes

  (i)    one read of 4 KiB at a random offset in each block;
  (ii)   16 reads of 256 B per block on average, at random positions anywhere;
  (iii)  one read of the whole buffer;
  (iv)   1024 reads of 16 B per block on average, anywhere (2^20 at 64 MiB);

and per shape the contenders

  (a)  one Decoder.read_blocks call: a block is decoded from its root once
       per read that touches it.  At (iv) with --reps-a-iv repetitions;
  (b)  Decoder.decode_batch_items of the distinct touched blocks into a
       scratch buffer, then one gather (bench_blocks_read.py's);
  (g)  one Decoder.gather_blocks call: every touched block walked once.

The contenders alternate in one process; a figure is the median of --reps
runs after --warmup, device events around the call(s); the whole series is
repeated --series times and the medians' range is the spread.  Every output
is compared with the text's slices before anything is timed.  Exit status 1
when an output is wrong, or (g) at (ii) is not faster than (a) by more than
the sum of their spreads.

    python tools/bench_blocks_gather.py [--reps 20] [--warmup 3] [--series 3] [--mib 64] [--block-kib 64]
        [--reps-a-iv 5] [--shapes i,ii,iii,iv] [--out profiles/blocks_gather_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import huffmandecoderongpus_amd as H  # noqa: E402
from huffmandecoderongpus_amd import synth  # noqa: E402
from bench_blocks_read import shapes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--block-kib", type=int, default=64)
    ap.add_argument("--reps-a-iv", type=int, default=5)
    ap.add_argument("--shapes", default="i,ii,iii,iv")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_blocks_gather: needs a GPU")
    tree = H.HuffFile.load(os.path.join(ROOT, "files", "kjv.txt.huff")).tree()
    kjv = synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1]
    n, B = a.mib << 20, a.block_kib << 10
    text = np.tile(kjv, n // kjv.size + 1)[:n]
    data, index = tree.encode_blocks(text, B)
    nb = index.shape[0]
    dec = H.Decoder(0)
    dec.set_tree(tree)
    d_data = torch.from_numpy(data).cuda()
    d_index = torch.from_numpy(index.view(np.int64)).cuda()
    d_text = torch.from_numpy(text).cuda()
    scratch = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(64)
    all_shapes = shapes(n, B, rng)                               # (i), (ii), (iii) as bench_blocks_read.py draws them
    all_shapes["iv"] = (rng.integers(0, n - 16 + 1, 1024 * nb), 16)
    rows = []
    for name in a.shapes.split(","):
        src, ln = all_shapes[name]
        m, total = src.size, src.size * ln
        reads = np.stack([src, np.full(m, ln, np.int64), np.arange(m, dtype=np.int64) * ln], axis=1)
        d_reads = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
        touched = np.unique(np.concatenate([src // B, (src + ln - 1) // B])) if name != "iii" else np.arange(nb)
        d_sub = d_index[torch.from_numpy(touched).cuda()].contiguous()
        d_src = torch.from_numpy(src).cuda()
        want = d_text if name == "iii" else d_text.as_strided((n - ln + 1, ln), (1, 1)).index_select(0, d_src).reshape(-1)
        out = {k: torch.zeros(total, dtype=torch.uint8, device="cuda") for k in "abg"}
        res = {k: (torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda"),
                   torch.zeros(6, dtype=torch.int32, device="cuda")) for k in "ag"}
        b_len = torch.zeros(touched.size, dtype=torch.int64, device="cuda")
        b_st = torch.zeros(touched.size, dtype=torch.int32, device="cuda")
        rows_view = scratch.as_strided((n - ln + 1, ln), (1, 1))

        def fa():
            dec.read_blocks(d_data, d_index, n, B, d_reads, out["a"], *res["a"])

        def fg():
            dec.gather_blocks(d_data, d_index, n, B, d_reads, out["g"], *res["g"])

        def fb():
            dec.decode_batch_items(d_data, d_sub, scratch, b_len, b_st)
            if name == "iii":
                out["b"].copy_(scratch)
            else:
                torch.index_select(rows_view, 0, d_src, out=out["b"].view(m, ln))

        paths = [("a", fa), ("b", fb), ("g", fg)]
        ok = True
        for k, fn in paths:                                      # one checked run of each
            scratch.zero_()
            fn()
            torch.cuda.synchronize()
            ok = ok and torch.equal(out[k], want)
        for k in "ag":
            summ = dec.batch_summary(res[k][2])
            ok = ok and summ["n_failed"] == 0 and summ["total_len"] == total and not res[k][1].any().item() \
                and bool((res[k][0] == ln).all().item())
        ok = ok and not b_st.any().item()
        reps = {k: a.reps_a_iv if (k, name) == ("a", "iv") else a.reps for k, _ in paths}
        med = {k: [] for k, _ in paths}
        for _ in range(a.series):
            ms = {k: [] for k, _ in paths}
            for i in range(a.warmup + a.reps):
                for k, fn in paths:                              # (alternating)
                    if i >= a.warmup + reps[k]:
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        ms[k].append(e0.elapsed_time(e1))
            for k in ms:
                med[k].append(statistics.median(ms[k]))
        row = {"shape": name, "reads": m, "read_bytes": ln, "blocks": nb, "touched_blocks": int(touched.size),
               "block_kib": a.block_kib, "text_mib": a.mib, "ok": ok, "round_tiles": dec.batch_round_tiles(),
               "reps": reps}
        for k in med:
            row[k + "_ms"] = round(statistics.median(med[k]), 4)
            row[k + "_series"] = [round(v, 4) for v in med[k]]
            row[k + "_spread_ms"] = round(max(med[k]) - min(med[k]), 4)
        row["a_minus_g_ms"] = round(row["a_ms"] - row["g_ms"], 4)
        row["g_minus_b_ms"] = round(row["g_ms"] - row["b_ms"], 4)
        row["g_faster_than_a"] = row["a_ms"] - row["g_ms"] > row["a_spread_ms"] + row["g_spread_ms"]
        rows.append(row)
        del out, want, d_reads, res
        torch.cuda.empty_cache()
    dec.close()
    result = {"bench": "blocks_gather", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
              "series": a.series,
              "protocol": "median of reps after warmup, device events around each contender's call(s), contenders "
                          "alternating; spread: range of the series' medians", "rows": rows}
    line = json.dumps(result)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cond = [r for r in rows if r["shape"] == "ii"]
    return 0 if all(r["ok"] for r in rows) and all(r["g_faster_than_a"] for r in cond) else 1


if __name__ == "__main__":
    sys.exit(main())
