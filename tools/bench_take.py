"""Record-take timing: one text cut into records (Encoder.encode_ragged, once
per shape), everything resident in HBM, the records decoded back by

  (t) take_ms    Decoder.take_records with ids=None (hh_decode_batch_take);
  (a) items_ms   Decoder.decode_batch_items on the same device list (it writes
                 the same bytes: a row's out_off is the record's offset);
  (c) single_ms  one Decoder.decode_device of the whole text encoded as a
                 single stream: the floor.

Shapes (the text is kjv.txt tiled to --mib MiB, kjv's code; tools/
bench_encode_ragged.py's):
  i    records of 64 KiB;
  ii   records of random length 1..127 (about 2^20 of them in 64 MiB);
  iii  lengths drawn log-uniform from 1 to 64 KiB;
  iv   on ii's buffer, 65536 random ids: (t) against (a'), decode_batch_items
       on a list whose rows were gathered and whose out_off was rewritten
       with torch outside the timed region.

Every figure is the median of --reps runs after --warmup, timed with device
events around the call on the current stream; the contenders alternate in one
process, --series times over; a figure is the median of the series' medians,
its spread their range.  Every output is compared with the text before
anything is timed.

    python tools/bench_take.py [--out profiles/take_bench.json] [--shapes i,ii,iii,iv]
    python tools/bench_take.py --shapes ii --only t      (for a kernel trace)
"""
import argparse
import ctypes as C
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
from bench_encode_ragged import offsets, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--shapes", default="i,ii,iii,iv")
    ap.add_argument("--only", default=None, help="time only this contender: t, a or c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 (the median's protocol)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_take: needs a GPU")
    hf = H.HuffFile.load(os.path.join(ROOT, "files", "kjv.txt.huff"))
    tree = hf.tree()
    kjv = synth.load_source(os.path.join(ROOT, "files"), "kjv.txt")[1]
    n = a.mib << 20
    text = np.tile(kjv, n // kjv.size + 1)[:n]
    d_text = torch.from_numpy(text).cuda()
    enc = H.Encoder(0)
    dec = H.Decoder(0)
    dec.set_tree(tree)
    rng = np.random.default_rng(2024)
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    # (c): the whole text as one stream
    cap1 = int(H.lib().hh_encode_bound(C.byref(tree._c), n))
    one = torch.zeros(cap1 + H.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
    bits1 = enc.encode(tree, d_text, one[:cap1])

    def single():
        return dec.decode_device(one, bits1, back)

    ok_c = single() == n and torch.equal(back, d_text)
    rows, kept = [], {}
    for shape in a.shapes.split(","):
        src = "ii" if shape == "iv" else shape
        if src in kept:
            offs, data, t = kept[src]
        else:
            offs = offsets(src, n, rng)
            nrec = offs.size - 1
            d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
            cap = H.encode_ragged_bound(tree, n, nrec)
            buf = torch.zeros(cap + H.PAYLOAD_PAD, dtype=torch.uint8, device="cuda")
            t = torch.empty((nrec, 4), dtype=torch.int64, device="cuda")
            _, total = enc.encode_ragged(tree, d_text, d_offs, buf[:cap], items_out=t, host_items=False)
            data = buf[: total + H.PAYLOAD_PAD]
            kept = {src: (offs, data, t)}
        nrec = offs.size - 1
        if shape != "iv":
            ids, items, want, m, nout = None, t, d_text, nrec, n
        else:
            m = 65536
            h_ids = rng.integers(0, nrec, size=m)
            ids = torch.from_numpy(h_ids).cuda()
            lens = (offs[1:] - offs[:-1]).astype(np.int64)[h_ids]
            o = np.concatenate([[0], np.cumsum(lens)])
            nout = int(o[-1])
            items = t[ids].clone()
            items[:, 2] = torch.from_numpy(o[:-1]).cuda()
            want = torch.from_numpy(np.concatenate([text[int(offs[r]): int(offs[r + 1])] for r in h_ids])).cuda()
        out = back[:nout]
        o_t = torch.empty(m + 1, dtype=torch.int64, device="cuda")
        s_t = torch.empty(m, dtype=torch.int32, device="cuda")
        l_a = torch.empty(m, dtype=torch.int64, device="cuda")
        s_a = torch.empty(m, dtype=torch.int32, device="cuda")

        def take():
            return dec.take_records(data, t, ids, out, out_offs=o_t, status=s_t)

        def batch():
            return dec.decode_batch_items(data, items, out, out_len=l_a, status=s_a)

        ok = bool(ok_c)
        for f, st in ((take, s_t), (batch, s_a)):
            out.zero_()
            f()
            torch.cuda.synchronize()
            ok = ok and int(st.ne(0).sum()) == 0 and torch.equal(out, want)
        ok = ok and int(o_t[-1]) == nout and torch.equal(o_t[1:] - o_t[:-1], l_a)
        contenders = {"t": take, "a": batch}
        if shape != "iv":
            contenders["c"] = single
        if a.only:
            contenders = {k: f for k, f in contenders.items() if k == a.only}
        med = {k: [] for k in contenders}
        for _ in range(a.series):
            for k, f in contenders.items():
                med[k].append(timed(f, a.reps, a.warmup))
        row = {"shape": shape, "records": int(nrec), "taken": int(m), "out_bytes": int(nout), "text_mib": a.mib,
               "ok": bool(ok), "take_tiles": dec.take_round_tiles(), "batch_tiles": dec.batch_round_tiles()}
        for k, v in med.items():
            row[f"{k}_ms"] = round(statistics.median(v), 4)
            row[f"{k}_spread_ms"] = round(max(v) - min(v), 4)
        for k in med:
            if k != "t" and "t" in med:
                row[f"t_over_{k}"] = round(statistics.median(med["t"]) / statistics.median(med[k]), 4)
        if "t" in med:
            row["t_gbs_out"] = round(nout / statistics.median(med["t"]) * 1e-6, 1)
        rows.append(row)
        torch.cuda.empty_cache()
    dec.close()
    enc.close()
    res = {"bench": "take", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "series": a.series,
           "protocol": "median of reps per series, device events around each call, contenders alternating; "
                       "figure = median of the series' medians, spread = their range", "rows": rows}
    by = {r["shape"]: r for r in rows}
    if "ii" in by and "t_over_a" in by["ii"]:
        res["condition_ii_t_at_most_a_tenth_of_a"] = by["ii"]["t_over_a"] <= 0.1
    if "i" in by and "t_over_a" in by["i"]:
        res["condition_i_t_at_most_1_5_a"] = by["i"]["t_over_a"] <= 1.5
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
