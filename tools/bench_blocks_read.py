"""Range reads from a block-coded buffer (hh_decode_blocks_read) against what
a caller does without them, by the protocol of tools/bench_batch_items.py:
kjv.txt tiled to --mib MiB in blocks of --block-kib KiB under one shared
code, everything resident in HBM.  Three shapes of reads

  (i)    one read of 4 KiB at a random offset in each block;
  (ii)   16 reads of 256 B per block on average, at random positions anywhere;
  (iii)  one read of the whole buffer;

and per shape the contenders

  (a)  one Decoder.read_blocks call;
  (b)  Decoder.decode_batch_items of the distinct touched blocks into a
       scratch buffer, then one gather of the ranges: the reads of a shape
       have one length, so the gather is one index_select of rows of an
       overlapping (n - len + 1, len) view of the scratch (one index per read,
       whole rows copied); for (iii) a plain copy;
  (c)  for (iii) only: decode_batch_items of all blocks in place.

The contenders alternate in one process; a figure is the median of --reps
runs after --warmup, device events around the call(s); the whole series is
repeated --series times and the medians' range is the spread.  Every output
is compared with the text's slices before anything is timed.

    python tools/bench_blocks_read.py [--reps 20] [--warmup 3] [--series 3] [--mib 64] [--block-kib 64]
        [--only a|b|c] [--out profiles/blocks_read_bench.json]
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


def shapes(n, B, rng):
    """name -> (src_off, len) arrays; destinations are packed in read order."""
    nb = n // B
    one = np.arange(nb, dtype=np.int64) * B + rng.integers(0, B - 4096 + 1, nb)
    return {"i": (one, 4096), "ii": (rng.integers(0, n - 256 + 1, 16 * nb), 256), "iii": (np.zeros(1, np.int64), n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--block-kib", type=int, default=64)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_blocks_read: needs a GPU")
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
    rows = []
    for name, (src, ln) in shapes(n, B, np.random.default_rng(64)).items():
        m, total = src.size, src.size * ln
        reads = np.stack([src, np.full(m, ln, np.int64), np.arange(m, dtype=np.int64) * ln], axis=1)
        d_reads = torch.from_numpy(np.ascontiguousarray(reads)).cuda()
        touched = np.unique(np.concatenate([src // B, (src + ln - 1) // B])) if name != "iii" else np.arange(nb)
        d_sub = d_index[torch.from_numpy(touched).cuda()].contiguous()
        d_src = torch.from_numpy(src).cuda()
        want = d_text if name == "iii" else d_text.as_strided((n - ln + 1, ln), (1, 1)).index_select(0, d_src).reshape(-1)
        out = {k: torch.zeros(total, dtype=torch.uint8, device="cuda") for k in "abc"}
        r_len = torch.zeros(m, dtype=torch.int64, device="cuda")
        r_st = torch.zeros(m, dtype=torch.int32, device="cuda")
        r_sum = torch.zeros(6, dtype=torch.int32, device="cuda")
        b_len = torch.zeros(touched.size, dtype=torch.int64, device="cuda")
        b_st = torch.zeros(touched.size, dtype=torch.int32, device="cuda")
        c_len = torch.zeros(nb, dtype=torch.int64, device="cuda")
        c_st = torch.zeros(nb, dtype=torch.int32, device="cuda")
        rows_view = scratch.as_strided((n - ln + 1, ln), (1, 1))

        def fa():
            dec.read_blocks(d_data, d_index, n, B, d_reads, out["a"], r_len, r_st, r_sum)

        def fb():
            dec.decode_batch_items(d_data, d_sub, scratch, b_len, b_st)
            if name == "iii":
                out["b"].copy_(scratch)
            else:
                torch.index_select(rows_view, 0, d_src, out=out["b"].view(m, ln))

        def fc():
            dec.decode_batch_items(d_data, d_index, out["c"], c_len, c_st)

        paths = [("a", fa), ("b", fb)] + ([("c", fc)] if name == "iii" else [])
        ok = True
        for k, fn in paths:                                      # one checked run of each
            scratch.zero_()
            fn()
            torch.cuda.synchronize()
            ok = ok and torch.equal(out[k], want)
        summ = dec.batch_summary(r_sum)
        ok = ok and summ["n_failed"] == 0 and summ["total_len"] == total and not r_st.any().item() \
            and bool((r_len == ln).all().item()) and not b_st.any().item()
        paths = [p for p in paths if a.only in (None, p[0])]
        med = {k: [] for k, _ in paths}
        for _ in range(a.series):
            ms = {k: [] for k, _ in paths}
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
        row = {"shape": name, "reads": m, "read_bytes": ln, "blocks": nb, "touched_blocks": int(touched.size),
               "block_kib": a.block_kib, "text_mib": a.mib, "ok": ok, "round_tiles": dec.batch_round_tiles()}
        for k in med:
            row[k + "_ms"] = round(statistics.median(med[k]), 4)
            row[k + "_series"] = [round(v, 4) for v in med[k]]
            row[k + "_spread_ms"] = round(max(med[k]) - min(med[k]), 4)
        if "a" in med and "b" in med:
            row["a_minus_b_ms"] = round(row["a_ms"] - row["b_ms"], 4)
            row["a_no_longer_than_b"] = row["a_ms"] <= row["b_ms"] + max(row["a_spread_ms"], row["b_spread_ms"])
        rows.append(row)
        del out, want, d_reads
        torch.cuda.empty_cache()
    dec.close()
    res = {"bench": "blocks_read", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "series": a.series, "only": a.only,
           "protocol": "median of reps after warmup, device events around each contender's call(s), contenders "
                       "alternating; spread: range of the series' medians", "rows": rows}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    cond = [r for r in rows if r["shape"] == "i" and "a_no_longer_than_b" in r]
    return 0 if all(r["ok"] for r in rows) and all(r["a_no_longer_than_b"] for r in cond) else 1


if __name__ == "__main__":
    sys.exit(main())
