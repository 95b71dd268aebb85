"""A file-driven miBF build next to the in-memory stages on the same reads: the reads of tools/mibf_bench.py's shape
(synthetic 150-base reads, C5 spaced seeds, k = 31, the same bit vector size) written as ONE FASTA file under the system
temp directory, then MIBloomFilter.buildFromFiles (an id per record, uint32 ids, parallel saturation per 64 MiB batch,
32 GiB of scratch) twice -- the second build is the number -- and, for comparison in the same process, insertFile of that
file into a filter of the same size and the in-memory insertSeqs / insertIDs / insertSaturation over the same reads and
ids.  Prints one JSON line: per pass seconds, the parser's seconds and Gk-mers/s.
    python tools/mibf_build_probe.py [n_reads] [scratch_GiB]
Run each probe in a process of its own."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import btl_bloomfilter_amd as m
from mibf_bench import C5_SEEDS, calc_optimal_size, timed


def write_fasta(path, reads, L):
    """>r / the read, one record per read: (n, 3 + L + 1) bytes written at once"""
    a = reads.cpu().numpy().reshape(-1, L)
    rec = np.empty((a.shape[0], L + 4), np.uint8)
    rec[:, :3] = np.frombuffer(b">r\n", np.uint8)
    rec[:, 3:3 + L] = a
    rec[:, 3 + L] = ord("\n")
    rec.tofile(path)


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
    scratch = int(float(sys.argv[2]) * (1 << 30)) if len(sys.argv) > 2 else 32 << 30
    k, h, L = 31, 4, 150
    kmers = n_reads * (L - k + 1)
    bits = calc_optimal_size(1.2e9, 0.5, h)
    reads = m.synth_reads_device(42, 0, n_reads, L)
    fd, path = tempfile.mkstemp(suffix=".fa", prefix="mibf_build_probe_")
    os.close(fd)
    try:
        write_fasta(path, reads, L)
        res = {"n_reads": n_reads, "kmers": kmers, "bits": bits, "file_bytes": os.path.getsize(path)}
        for run in ("first", "second"):
            t = time.perf_counter()
            mi, f, rep = m.MIBloomFilter.buildFromFiles([path], k, seeds=C5_SEEDS, id_bytes=4, bits=bits, ids="record",
                                                        saturation="parallel", scratch_bytes=scratch)
            res[run] = {"wall_s": round(time.perf_counter() - t, 4), "seconds": [round(x, 4) for x in rep["seconds"]],
                        "seconds_parse": [round(x, 4) for x in rep["seconds_parse"]], "batches": rep["batches"],
                        "gkmers_per_s": [round(kmers / x / 1e9, 3) if x else None for x in rep["seconds"]],
                        "saturate": rep["sat_counts4"], "pop": rep["pop"]}
            mi.close()
            f.close()
        # pass 0 alone, and insertFile (its byte-range readers: what pass 1 would be with them)
        t_cnt, cnt = timed(lambda: m.countWindowsFile(path, k, whole=True))
        f = m.BloomFilter(bits, h, k)
        f.setSpacedSeeds(C5_SEEDS, 1)
        t_file, st = timed(lambda: f.insertFile(path))
        f.close()
        # the in-memory stages on the same reads and ids
        ids = (torch.arange(n_reads, device="cuda", dtype=torch.int64) + 1).to(torch.int32)
        f = m.BloomFilter(bits, h, k)
        f.setSpacedSeeds(C5_SEEDS, 1)
        t_bv, _ = timed(lambda: f.insertSeqs(reads, read_len=L))
        mi = m.MIBloomFilter(f, 4)
        mi.setScratchBudget(scratch)
        t_ins, _ = timed(lambda: mi.insertIDs(reads, ids, read_len=L))
        t_sat, sat = timed(lambda: mi.insertSaturation(reads, ids, read_len=L))
        res["count_file"] = {"ms": round(t_cnt, 2), "clean_windows": cnt["n_windows"], "parse_s": round(cnt["seconds_parse"], 4)}
        res["insert_file"] = {"ms": round(t_file, 2), "parse_s": round(st["seconds_parse"], 4)}
        res["in_memory_ms"] = {"stage1_insert": round(t_bv, 2), "insert_ids": round(t_ins, 2), "saturate_parallel": round(t_sat, 2)}
        res["in_memory_gkmers_per_s"] = {kk: round(kmers / v / 1e6, 3) for kk, v in res["in_memory_ms"].items()}
        res["in_memory_saturate"] = sat
    finally:
        os.unlink(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
