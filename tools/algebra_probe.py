"""Bytes per second of the filter algebra against the streaming readers it is modelled on (not on the product path):

    python tools/algebra_probe.py [--log2-bits 39] [--log2-bits-4src 38] [--log2-counters 36] [--runs 5] [--out FILE]

times, on filters of 2^log2-bits bits, btlbf_digest (N bytes read) and btlbf_compare (2 N) -- the yardsticks --
btlbf_combine with 1 source (3 N: two reads, one write) and with 4 (6 N; five filters of 2^39 bits do not fit one MI355X,
hence its own size), btlbf_fold by 2 and by 2^20 (N (1 + 1 / factor); the latter takes the two-stage plan) and
btlbf_threshold_bits on 2^log2-counters byte counters (N + N / 8).  Every call is synchronous (it ends in a device
synchronise), so a host clock around it is the call's time; one warm-up call, then --runs timed ones; the median and the
best are reported.  fold and threshold allocate their result inside the call: the time to create (and so allocate) an
equal filter is measured the same way and reported next to them, and `net` is the call minus that.  Prints one JSON line
per operation and, last, one with the ratios to digest."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, K, L = 3, 25, 150


def timed(fn, runs, cleanup=None):
    out = []
    for i in range(runs + 1):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        if cleanup:
            cleanup(r)
        if i:
            out.append(dt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bits", type=int, default=39)
    ap.add_argument("--log2-bits-4src", type=int, default=38)
    ap.add_argument("--log2-counters", type=int, default=36)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "the probe needs a GPU"
    import btl_bloomfilter_amd as m

    reads = m.synth_reads_device(1, 0, 1 << 18, L)  # contents for the arrays; the rates do not depend on them
    results = {}
    lines = []

    def report(name, nbytes_moved, times, alloc=None):
        med, best = statistics.median(times), min(times)
        row = {"op": name, "bytes_moved": nbytes_moved, "median_s": med, "best_s": best, "GBps_median": nbytes_moved / med / 1e9,
               "GBps_best": nbytes_moved / best / 1e9, "runs": len(times)}
        if alloc is not None:
            net = max(med - alloc, 1e-9)
            row.update({"create_equal_filter_s": alloc, "GBps_net": nbytes_moved / net / 1e9})
        results[name] = row
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    def bit_filter(log2_bits):
        f = m.BloomFilter(1 << log2_bits, H, K)
        f.setInsertMode("direct")  # no pipeline scratch next to arrays of this size
        f.insertSeqs(reads, read_len=L)
        return f

    n = (1 << a.log2_bits) // 8
    x, y = bit_filter(a.log2_bits), bit_filter(a.log2_bits)
    report("digest", n, timed(x.digest, a.runs))
    report("compare", 2 * n, timed(lambda: x.compare(y), a.runs))
    report("combine_1", 3 * n, timed(lambda: x.combine([y], "or"), a.runs))
    del y
    for factor in (2, 1 << 20):
        alloc = statistics.median(timed(lambda: m.BloomFilter((1 << a.log2_bits) // factor, H, K), a.runs, lambda f: f.close()))
        report("fold_%d" % factor, n + n // factor, timed(lambda: x.fold(factor), a.runs, lambda f: f.close()), alloc)
    del x
    torch.cuda.empty_cache()
    n4 = (1 << a.log2_bits_4src) // 8
    fs = [bit_filter(a.log2_bits_4src) for _ in range(5)]
    report("digest_at_4src_size", n4, timed(fs[0].digest, a.runs))
    report("combine_4", 6 * n4, timed(lambda: fs[0].combine(fs[1:], "or"), a.runs))
    del fs
    nc = 1 << a.log2_counters
    c = m.CountingBloomFilter(nc, H, K, countThreshold=2)
    c.setInsertMode("direct")
    c.insertSeqs(reads, read_len=L, increment_all=True)
    alloc = statistics.median(timed(lambda: m.BloomFilter(nc, H, K), a.runs, lambda f: f.close()))
    report("digest_counters", nc, timed(c.digest, a.runs))
    report("threshold_u8", nc + nc // 8, timed(lambda: c.toBloomFilter(2), a.runs, lambda f: f.close()), alloc)
    base = results["digest"]["GBps_median"]
    ratios = {k: round((v.get("GBps_net") or v["GBps_median"]) / base, 3) for k, v in results.items()}
    lines.append(json.dumps({"ratio_to_digest": ratios, "fold_2^20_over_fold_2_time_per_byte":
                             round(results["fold_2"]["GBps_net"] / results["fold_1048576"]["GBps_net"], 3)}))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
