"""Read classification from a FASTQ file against its two ingredients, on the C5 miBF of tools/classify_pair_probe.py
(k = 31, 4 spaced seeds, uint16 ids, ids = read index / 10^4 + 1): 2^21 synthetic 150-base reads written as plain FASTQ.
One process, a warm-up of each, then --reps rounds (default 2: the spread) of
  (a)  classify on those reads resident in HBM (one call, device tables and results);
  (b)  the sequential parser alone over the file (btlbf_fastx_open / _next with BTLBF_FASTX_WHOLE, pinned batches of the
       classifier's size, no GPU work); and its open + close alone, the pinned allocations every run of (b), (c), (c')
       pays before the first base is parsed;
  (a_batched) as (a), one classify call per batch of the file classifier's size;
  (c)  classifyFile(summary_only=True): parse, copy, classify, tally; only the summary leaves the GPU;
  (c') classifyFile with per-row results copied out batch by batch.
Wall-clock seconds of every call; the file is read from the page cache after the warm-up.  The pipeline overlaps when
(c) is below (a) + (b) by more than the spread of the repetitions; expect about max(a, b) plus the first batch's latency.
    python tools/classify_file_probe.py [--reads N] [--reps R] [--limit L] [--batch-bytes B] [--dir D] [--json OUT]
    python tools/classify_file_probe.py --two-files      # one summary over two files of N / 2 mates each (for a
                                                          # kernel trace: interleave and tally next to classify)"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]


def write_fastq(path, reads, L):
    """reads: uint8 [n, L] -> 4-line FASTQ records of fixed length, written with numpy"""
    n = reads.shape[0]
    rec = np.empty((n, 3 + L + 3 + L + 1), np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", np.uint8)
    rec[:, 3:3 + L] = reads
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = ord("I")
    rec[:, 6 + 2 * L] = ord("\n")
    rec.tofile(path)


def parse_only(m, path, k, batch_bytes, open_only=False):
    L = m._lib.load()
    r = C.c_void_p()
    m._lib.check(L.btlbf_fastx_open(C.byref(r), path.encode(), m._lib.FASTX_WHOLE, k, batch_bytes))
    n_seqs = n_batches = 0
    try:
        while not open_only:
            b, s = C.c_void_p(), C.c_void_p()
            nb, ns = C.c_uint64(), C.c_uint64()
            m._lib.check(L.btlbf_fastx_next(r, C.byref(b), C.byref(nb), C.byref(s), C.byref(ns)))
            if ns.value == 0:
                return n_seqs, n_batches
            n_seqs += ns.value
            n_batches += 1
        return 0, 0
    finally:
        L.btlbf_fastx_close(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=2, help="extra_frame_limit (1073741824: the full walk)")
    ap.add_argument("--batch-bytes", type=int, default=64 << 20)
    ap.add_argument("--scratch-gib", type=float, default=8)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--two-files", action="store_true")
    a = ap.parse_args()
    import torch

    import btl_bloomfilter_amd as m

    k, h, L = 31, 4, 150
    n_reads = a.reads
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
    prob_h, minc_h = np.full(n_ids, 1e-3), np.ones(n_ids, np.uint32)
    kw = dict(extra_frame_limit=a.limit, max_results=4)
    tmp = a.dir or tempfile.mkdtemp(prefix="classify_file_probe_")
    host = reads.cpu().numpy().reshape(n_reads, L)
    res = {"reads": n_reads, "read_len": L, "limit": a.limit, "batch_bytes": a.batch_bytes}
    if a.two_files:
        p1, p2 = os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")
        write_fastq(p1, host[0::2], L)
        write_fastq(p2, host[1::2], L)
        t0 = time.perf_counter()
        best, any_, totals = mi.classifyFile(p1, prob_h, minc_h, path2=p2, batch_bytes=a.batch_bytes, summary_only=True, **kw)
        res.update(two_files_s=round(time.perf_counter() - t0, 4), totals=totals.tolist())
        print(json.dumps(res))
        os.remove(p1)
        os.remove(p2)
        return
    path = os.path.join(tmp, "reads.fq")
    write_fastq(path, host, L)
    res["file_bytes"] = os.path.getsize(path)
    prob = torch.from_numpy(prob_h).cuda()
    minc = torch.from_numpy(minc_h.astype(np.int32)).cuda()

    def resident():
        out = mi.classify(reads, prob, minc, read_len=L, **kw)
        torch.cuda.synchronize()
        return int((out[1] > 0).sum())

    def per_row():
        rows = with_hits = 0
        for first, hits, n, sat, ev in mi.classifyFile(path, prob_h, minc_h, batch_bytes=a.batch_bytes, **kw):
            assert first == rows
            rows += len(n)
            with_hits += int((n > 0).sum())
        assert rows == n_reads
        return with_hits

    def summary():
        best, any_, totals = mi.classifyFile(path, prob_h, minc_h, batch_bytes=a.batch_bytes, summary_only=True, **kw)
        assert totals[0] == n_reads
        return int(totals[0] - totals[1])

    def resident_batched():  # (a) cut as the file classifier cuts it: one classify call per batch of whole reads
        per = a.batch_bytes // L
        hit = 0
        for r0 in range(0, n_reads, per):
            out = mi.classify(reads[r0 * L:(r0 + per) * L], prob, minc, read_len=L, **kw)
            hit += int((out[1] > 0).sum())
        torch.cuda.synchronize()
        return hit

    calls = {"a_resident": resident, "a_resident_batched": resident_batched,
             "b_parse": lambda: parse_only(m, path, k, a.batch_bytes)[0],
             "b_open_close_only": lambda: parse_only(m, path, k, a.batch_bytes, True)[0], "c_summary": summary,
             "c_rows": per_row}
    res["seconds"] = {name: [] for name in calls}
    check = {name: fn() for name, fn in calls.items()}  # warm-up of each; every path sees the same reads
    assert check["b_parse"] == n_reads, check
    assert check["a_resident"] == check["a_resident_batched"] == check["c_summary"] == check["c_rows"], check
    res["rows_with_hits"] = check["a_resident"]
    for _ in range(a.reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            res["seconds"][name].append(round(time.perf_counter() - t0, 4))
    s = res["seconds"]
    spread = max(max(v) - min(v) for v in s.values())
    res["spread_s"] = round(spread, 4)
    res["a_plus_b_minus_c_s"] = round(min(s["a_resident"]) + min(s["b_parse"]) - max(s["c_summary"]), 4)
    res["overlap"] = bool(res["a_plus_b_minus_c_s"] > spread)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as out:
            json.dump(res, out, indent=1)
            out.write("\n")
    os.remove(path)


if __name__ == "__main__":
    main()
