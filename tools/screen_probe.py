"""The read screen against the loop it replaces, on one build: 2^21 synthetic 150-base reads resident in HBM, k = 31,
h = 4, F in {1, 2, 4, 8} bit filters about 30 % full (each holds other synthetic reads of a seed of its own, so the
screened reads miss -- a first probe finds its bit set in about three cases of ten), in two regimes: filters of 2^28 bits
(32 MiB each: cache-resident) and of 2^36 bits (8 GiB each: every probe is an HBM gather).  Timed in one process and
alternating, with device events around whole calls after a warm-up of each:
    screen        screenSeqs(filters[:F], reads)
    loop_direct   F x (containsSeqs + count_per_seq), the filters' query mode DIRECT
    loop_auto     the same, query mode AUTO
First `screen` runs twice more on its own: the spread of identical calls.  A difference inside twice that spread is
none.  Prints one JSON line per (regime, F) with the ms of every repetition, the medians, and the k-mers per second of
`screen`; the three paths' results are compared on the way (hits and valid must be equal).
    python tools/screen_probe.py [--log-bits 28,36] [--filters 1,2,4,8] [--reads N] [--reps R] [--fill 0.3]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-bits", default="28,36")
    ap.add_argument("--filters", default="1,2,4,8")
    ap.add_argument("--reads", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fill", type=float, default=0.3)
    a = ap.parse_args()
    import torch

    import btl_bloomfilter_amd as m

    assert torch.cuda.is_available(), "the probe measures on a GPU; there is nothing to fall back to"
    k, h, L = 31, 4, 150
    counts = [int(x) for x in a.filters.split(",")]
    reads = m.synth_reads_device(7, 0, a.reads, L)
    n_bytes = a.reads * L
    kmers = a.reads * (L - k + 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def loop(fs):
        cols, valid = [], None
        for f in fs:
            hit, ok, _ = f.containsSeqs(reads, read_len=L)
            hj, valid = m.count_per_seq(hit, ok, n_bytes, k, read_len=L)
            cols.append(hj)
        return torch.stack(cols, dim=1), valid

    for log_bits in [int(x) for x in a.log_bits.split(",")]:
        bits = 1 << log_bits
        # fill = 1 - exp(-n h / m)  ->  n k-mers to insert, in chunks of whole reads
        n_ins = int(-math.log(1.0 - a.fill) * bits / h / (L - k + 1))
        filters = []
        for j in range(max(counts)):
            f = m.BloomFilter(bits, h, k)
            done = 0
            while done < n_ins:
                n = min(1 << 22, n_ins - done)
                f.insertSeqs(m.synth_reads_device(1000 + j, done, n, L), read_len=L)
                done += n
            filters.append(f)
        torch.cuda.synchronize()
        pop = [f.getPop() / bits for f in filters]
        for nf in counts:
            fs = filters[:nf]

            def set_mode(mode):
                for f in fs:
                    f.setQueryMode(mode)

            calls = {"screen": lambda: m.screenSeqs(fs, reads, read_len=L)[:2],
                     "loop_direct": lambda: (set_mode("direct"), loop(fs))[1],
                     "loop_auto": lambda: (set_mode("auto"), loop(fs))[1]}
            res = {"log_bits": log_bits, "filters": nf, "reads": a.reads, "kmers": kmers, "fill": [round(p, 4) for p in pop[:nf]],
                   "ms": {n: [] for n in calls}}
            outs = {}
            for name, fn in calls.items():  # warm-up of each, and the results compared
                _, outs[name] = timed(fn)
            for name in ("loop_direct", "loop_auto"):
                assert torch.equal(outs[name][0], outs["screen"][0]) and torch.equal(outs[name][1], outs["screen"][1]), name
            res["hit_fraction"] = round(float(outs["screen"][0].sum()) / (kmers * nf), 6)
            outs = None
            res["screen_alone_ms"] = [round(timed(calls["screen"])[0], 3) for _ in range(2)]
            for _ in range(a.reps):
                for name, fn in calls.items():
                    res["ms"][name].append(round(timed(fn)[0], 3))
            set_mode("auto")
            res["median_ms"] = {n: round(statistics.median(v), 3) for n, v in res["ms"].items()}
            res["spread_ms"] = round(max(res["ms"]["screen"] + res["screen_alone_ms"]) - min(res["ms"]["screen"] + res["screen_alone_ms"]), 3)
            res["screen_Gkmers_per_s"] = round(kmers / res["median_ms"]["screen"] / 1e6, 2)
            res["screen_Gprobes0_per_s"] = round(kmers * nf / res["median_ms"]["screen"] / 1e6, 2)
            print(json.dumps(res), flush=True)
        for f in filters:
            f.close()
        filters = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
