"""Read-pair classification against single-read classification of the same mates, on a C5 miBF (k = 31, 4 spaced seeds,
uint16 ids): 2^20 pairs of 150-base synthetic mates in device memory, ids = read index / 10^4 + 1, every table in LDS.
In one process and alternating, after a warm-up of each: classifyPairs over the interleaved buffer (2^20 rows) and
classify over the same 2^21 mates, timed with device events around the whole call (phase 1 included).  Prints one JSON
line with the ms of every repetition and their medians.
    python tools/classify_pair_probe.py [--pairs N] [--reps R] [--limit L] [--scratch-gib G] [--single-only]
--single-only times classify alone and lets the script run against a library built before the paired call existed
(BTLBF_LIB=<that libbtlbf.so>): the baseline for the single-read kernel.  Compare builds by running the two
alternately in one session, and the same build twice first: a difference inside twice that spread is none."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=2, help="extra_frame_limit (1073741824: the full walk)")
    ap.add_argument("--scratch-gib", type=float, default=8)
    ap.add_argument("--single-only", action="store_true")
    a = ap.parse_args()
    if a.single_only:  # an older library has no paired entry point: do not ask it for one
        from btl_bloomfilter_amd import _lib

        _lib._PROTOS.pop("btlbf_mibf_classify_pairs", None)
    import torch

    import btl_bloomfilter_amd as m

    k, h, L = 31, 4, 150
    n_reads = 2 * a.pairs
    entries = n_reads * (L - k + 1)
    v = int(-float(entries) * h / math.log(1.0 - 0.5 ** (1.0 / h)))  # BloomFilter::calcOptimalSize, fpr 0.5
    bits = v + (64 - v % 64)
    reads = m.synth_reads_device(42, 0, n_reads, L)
    ids = (torch.arange(n_reads, device="cuda", dtype=torch.int64) // 10_000 + 1).to(torch.int32)
    f = m.BloomFilter(bits, h, k)
    f.setSpacedSeeds(C5_SEEDS, 1)
    f.insertSeqs(reads, read_len=L)
    mi = m.MIBloomFilter(f, 2)
    f.close()
    mi.setScratchBudget(int(a.scratch_gib * (1 << 30)))
    mi.insertIDs(reads, ids, read_len=L)
    mi.insertSaturation(reads, ids, read_len=L)
    n_ids = n_reads // 10_000 + 2
    prob = torch.full((n_ids,), 1e-3, dtype=torch.float64, device="cuda")
    minc = torch.ones(n_ids, dtype=torch.int32, device="cuda")
    kw = dict(extra_frame_limit=a.limit, max_results=4, read_len=L)
    calls = {"classify": lambda: mi.classify(reads, prob, minc, **kw)}
    if not a.single_only:
        calls["classifyPairs"] = lambda: mi.classifyPairs(reads, prob, minc, **kw)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    res = {"pairs": a.pairs, "limit": a.limit, "scratch_GiB": a.scratch_gib, "lib": os.environ.get("BTLBF_LIB", "product"),
           "ms": {n: [] for n in calls}}
    for name, fn in calls.items():  # warm-up of each
        _, out = timed(fn)
        res[name + "_rows_with_hits"] = int((out[1] > 0).sum())
        res[name + "_eval_sum"] = int(out[3].to(torch.int64).sum())
        res[name + "_tables_lds_global"] = list(mi.classifyPaths())
        del out
    for _ in range(a.reps):
        for name, fn in calls.items():
            t, out = timed(fn)
            res["ms"][name].append(round(t, 3))
            del out
    res["median_ms"] = {n: round(statistics.median(v), 3) for n, v in res["ms"].items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
