"""diagnostic: rates of the DIRECT counting-filter kernels per counter width, side by side in one session:
    python tools/wide_cbf_probe.py [log2 counters, default 35] [hash count, default 3] [reads, default 2x10^7]
incrementAll, insert (incrementMin, parallel order) and query of synthetic 150 bp reads (k = 31, threshold 1) on a filter
of that many COUNTERS of 8, 16, 32 and 64 bits -- 8 bits through the direct 8-bit kernels (insert and query mode
"direct"), the others through wide_counter_kernels.hip.  A width whose array does not fit the HBM is reported and
skipped.  Every probe is one random HBM access whatever the width, so the expectation is parity per probe."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import btl_bloomfilter_amd as m
from btl_bloomfilter_amd import _lib

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 35
h = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n = int(float(sys.argv[3])) if len(sys.argv) > 3 else 20_000_000
L, k = 150, 31
reads = m.synth_reads_device(42, 0, n, L)
kmers = n * (L - k + 1)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
for bits in (8, 16, 32, 64):
    nbytes = (1 << lg) * bits // 8
    try:
        f = m.CountingBloomFilter(nbytes, h, k, 1, counter_bits=bits)
    except _lib.BtlbfError as e:
        print("bits=%d: 2^%d counters = %d GiB do not fit: %s" % (bits, lg, nbytes >> 30, e), flush=True)
        continue
    f.setInsertMode("direct")
    f.setQueryMode("direct")
    for rep in range(3):  # round 0 also zeroes the array and warms the code up; rounds 1 and 2 give the spread
        ev[0].record()
        f.insertSeqs(reads, read_len=L, increment_all=True)
        ev[1].record()
        f.insertSeqs(reads, read_len=L)
        ev[2].record()
        _, _, cnt = f.containsSeqs(reads, read_len=L, want_valid=False, want_counts=True)
        ev[3].record()
        torch.cuda.synchronize()
        t = [ev[i].elapsed_time(ev[i + 1]) for i in range(3)]
        print("bits=%d counters=2^%d h=%d round %d: incrementAll %.1f ms (%.2f G probes/s), insert %.1f ms (%.2f), "
              "query %.1f ms (%.2f); hits %d of %d" % ((bits, lg, h, rep) + tuple(
                  x for ms in t for x in (ms, kmers * h / ms / 1e6)) + (int(cnt[1]), int(cnt[0]))), flush=True)
    f.close()
    del f
    torch.cuda.empty_cache()
