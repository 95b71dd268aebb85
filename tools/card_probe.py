"""The cardinality sketch's fused kernel against its two yardsticks, on one build: 2 x 10^7 synthetic 150-base reads
resident in HBM (3 GB), k = 31.  Timed in one process and alternating, with device events around whole calls after a
warm-up of each, three rounds:
    card_s11_r22   KmerCardinality(31, 11, 22).addSeqs(reads)   one window in 2048 sampled: the hash stage and the mask
    card_s0_r22    KmerCardinality(31, 0, 22).addSeqs(reads)    every window sampled: one atomic per k-mer on 16 MiB
    count_windows  countWindows(reads, 31)                      no hashing: the bytes read once
    contains_h1    BloomFilter(2^33 bits, h = 1).containsSeqs(reads), query mode direct, the filter holding these reads:
                   the hash stage plus one gather per k-mer and the hit bitmap
Prints one JSON line: the ms of every repetition, the medians, the spread of each path (max - min of its repetitions)
and the G k-mers per second.  A difference inside twice the spread is none.  The sketches are checked on the way: the
clean windows equal countWindows', at sample_bits 0 the counters sum to them.
    python tools/card_probe.py [--reads N] [--rounds R] [--table-bits 22] [--log-bits 33]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table-bits", type=int, default=22)
    ap.add_argument("--log-bits", type=int, default=33)
    a = ap.parse_args()
    import torch

    import btl_bloomfilter_amd as m

    assert torch.cuda.is_available(), "the probe measures on a GPU; there is nothing to fall back to"
    k, L = 31, 150
    reads = m.synth_reads_device(7, 0, a.reads, L)
    kmers = a.reads * (L - k + 1)
    c11, c0 = m.KmerCardinality(k, 11, a.table_bits), m.KmerCardinality(k, 0, a.table_bits)
    f = m.BloomFilter(1 << a.log_bits, 1, k)
    f.setInsertMode("direct")
    f.setQueryMode("direct")
    f.insertSeqs(reads, read_len=L)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    calls = {"card_s11_r22": lambda: c11.addSeqs(reads, read_len=L),
             "card_s0_r22": lambda: c0.addSeqs(reads, read_len=L),
             "count_windows": lambda: m.countWindows(reads, k, read_len=L),
             "contains_h1": lambda: f.containsSeqs(reads, read_len=L, want_valid=False, want_counts=True)}
    res = {"reads": a.reads, "kmers": kmers, "table_bits": a.table_bits, "filter_log_bits": a.log_bits, "ms": {n: [] for n in calls}}
    outs = {name: timed(fn)[1] for name, fn in calls.items()}  # warm-up of each
    windows, clean = outs["count_windows"]
    assert windows == kmers and clean == kmers
    assert c11.totals()[:2] == (kmers, kmers) and c0.totals() == (kmers, kmers, kmers)
    assert int(c0.table().astype("uint64").sum()) == kmers
    assert int(outs["contains_h1"][2][1]) == kmers  # every k-mer is in the filter
    res["sampled_s11"] = c11.totals()[2]
    res["filter_fill"] = round(f.getPop() / float(1 << a.log_bits), 4)
    outs = None
    for _ in range(a.rounds):
        for name, fn in calls.items():
            res["ms"][name].append(round(timed(fn)[0], 3))
    res["median_ms"] = {n: round(statistics.median(v), 3) for n, v in res["ms"].items()}
    res["spread_ms"] = {n: round(max(v) - min(v), 3) for n, v in res["ms"].items()}
    res["Gkmers_per_s"] = {n: round(kmers / v / 1e6, 2) for n, v in res["median_ms"].items()}
    e = c11.estimate()
    res["estimate_s11"] = {"distinct": e.distinct, "singletons": e.singletons, "occupancy": round(e.occupancy, 4)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
