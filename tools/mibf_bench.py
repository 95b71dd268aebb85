"""miBF throughput on the issue's shape: 10^7 synthetic 150-base reads (1.2*10^9 k-mers), C5 spaced seeds, k = 31, a
stage-1 filter of calcOptimalSize(1.2e9 entries, fpr 0.5, 4 hashes) bits (a multiple of 64, not a power of two), ids =
read index / 10^4 + 1 as uint16.  Prints one JSON line: Gk-mers/s and ms per call of insert-IDs, parallel saturation
query (max_miss 0 and 1) and read classification (early stop after 2 extra frames, and the full walk), each timed once
after the stage-1 build.
    python tools/mibf_bench.py [n_reads] [scratch_GiB]
(per-kernel times: run it under rocprofv3 --kernel-trace --stats)"""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import btl_bloomfilter_amd as m

C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]


def calc_optimal_size(entries, fpr, h):
    """BloomFilter::calcOptimalSize (BloomFilter.hpp:406-413)"""
    v = int(-float(entries) * h / math.log(1.0 - fpr ** (1.0 / h)))
    return v + (64 - v % 64)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    scratch = float(sys.argv[2]) if len(sys.argv) > 2 else 32
    k, h, L = 31, 4, 150
    kmers = n_reads * (L - k + 1)
    bits = calc_optimal_size(1.2e9, 0.5, h)
    reads = m.synth_reads_device(42, 0, n_reads, L)
    ids = (torch.arange(n_reads, device="cuda", dtype=torch.int64) // 10_000 + 1).to(torch.int32)
    f = m.BloomFilter(bits, h, k)
    f.setSpacedSeeds(C5_SEEDS, 1)
    t_bv, _ = timed(lambda: f.insertSeqs(reads, read_len=L))
    t_create, mi = timed(lambda: m.MIBloomFilter(f, 2))
    mi.setScratchBudget(int(scratch * (1 << 30)))
    t_ins, _ = timed(lambda: mi.insertIDs(reads, ids, read_len=L))
    t_sat, sat = timed(lambda: mi.insertSaturation(reads, ids, read_len=L))
    res = {"n_reads": n_reads, "kmers": kmers, "bits": bits, "pop": mi.getPop(), "scratch_GiB": scratch,
           "ms": {"stage1_insert": round(t_bv, 2), "create": round(t_create, 2), "insert_ids": round(t_ins, 2),
                  "saturate_parallel": round(t_sat, 2)},
           "saturate": sat}
    for mx in (0, 1):
        t_q, out = timed(lambda: mi.query(reads, max_miss=mx, read_len=L, want_counts=True))
        res["ms"]["query_mm%d" % mx] = round(t_q, 2)
        res["query_mm%d_matched" % mx] = int(out[3][1])
        del out
    # classification of the same reads (MIBFQuerySupport::query per read): phase 1 is the query above, into scratch
    n_ids = n_reads // 10_000 + 2
    prob = torch.full((n_ids,), 1e-3, dtype=torch.float64, device="cuda")
    minc = torch.ones(n_ids, dtype=torch.int32, device="cuda")
    for lim in (2, 1 << 30):
        t_c, out = timed(lambda: mi.classify(reads, prob, minc, extra_frame_limit=lim, max_results=4, read_len=L))
        name = "classify_limit2" if lim == 2 else "classify_full_walk"
        res["ms"][name] = round(t_c, 2)
        res[name] = {"reads_per_s": round(n_reads / t_c * 1e3), "reads_with_hits": int((out[1] > 0).sum()),
                     "tables_lds_global": list(mi.classifyPaths())}
        del out
    res["query_mm0_reads_per_s"] = round(n_reads / res["ms"]["query_mm0"] * 1e3)
    res["gkmers_per_s"] = {kk: round(kmers / v / 1e6, 3) for kk, v in res["ms"].items() if kk not in ("create",)}
    res["pop_nonzero"], res["pop_saturated"] = mi.getPopNonZero(), mi.getPopSaturated()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
