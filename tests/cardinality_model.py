"""The k-mer cardinality sketch of include/btlbf.h (btlbf_card_*) restated in numpy: the model the CPU and GPU tests
hold the library to.  No test of its own.

Hashes come from the CPU oracle (oracle.pyoracle.Oracle.nthash_seq(seq, 1, k): the canonical ntHash value of every clean
window of one sequence); the mix, the sampling rule, the table, the totals, the histogram and the solver follow the
header's text.  accuracy_reads() is the input of the accuracy tests: a genome of 20 000 uniform random bases, 4 096 reads
of 100 bases at random offsets, 1 % substitutions, fixed seed."""
import math

import numpy as np

SAT = (1 << 32) - 1
U64 = np.uint64


def mix64(z):
    """the splitmix64 finaliser over a uint64 array (wrapping arithmetic)"""
    z = np.asarray(z, U64).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def split(buf, starts=None, read_len=0):
    """the sequences of a buffer under the three layouts of btlbf_layout"""
    buf = bytes(buf)
    if starts is not None:
        st = [int(x) for x in starts]
        return [buf[a:b] for a, b in zip(st[:-1], st[1:])]
    if read_len:
        assert len(buf) % read_len == 0
        return [buf[i:i + read_len] for i in range(0, len(buf), read_len)]
    return [buf]


def window_hashes(oracle, buf, k, starts=None, read_len=0):
    """-> (windows, canonical hashes of the clean windows, uint64)"""
    windows, hs = 0, []
    for s in split(buf, starts, read_len):
        windows += max(0, len(s) - k + 1)
        if len(s) >= k:
            hs.append(oracle.nthash_seq(s, 1, k)[1][:, 0])
    return windows, (np.concatenate(hs) if hs else np.zeros(0, U64)).astype(U64)


def buckets(hashes, sample_bits, table_bits):
    """the counters the sampled windows among `hashes` add to, one entry per sampled window"""
    z = mix64(hashes)
    if sample_bits:
        z = z[(z >> U64(64 - sample_bits)) == 0]
    return (z & U64((1 << table_bits) - 1)).astype(np.int64)


def add(table, totals, windows, hashes, sample_bits, table_bits):
    """the sketch after the windows are added -> (table uint32, totals uint64[3]); the inputs are not changed"""
    b = buckets(hashes, sample_bits, table_bits)
    t = table.astype(np.uint64) + np.bincount(b, minlength=1 << table_bits).astype(np.uint64)
    tot = np.asarray(totals, U64) + np.array([windows, hashes.size, b.size], U64)
    return np.minimum(t, U64(SAT)).astype(np.uint32), tot


def empty(table_bits):
    return np.zeros(1 << table_bits, np.uint32), np.zeros(3, U64)


def sketch(oracle, buf, k, sample_bits, table_bits, starts=None, read_len=0):
    w, h = window_hashes(oracle, buf, k, starts, read_len)
    return add(*empty(table_bits), w, h, sample_bits, table_bits)


def merge(a, b):
    (ta, na), (tb, nb) = a, b
    return np.minimum(ta.astype(U64) + tb.astype(U64), U64(SAT)).astype(np.uint32), np.asarray(na, U64) + np.asarray(nb, U64)


def histogram(table, n_hist):
    """t[i] = counters equal to i for i < n_hist - 1, t[n_hist - 1] = counters at or above it"""
    return np.bincount(np.minimum(table.astype(np.int64), n_hist - 1), minlength=n_hist).astype(U64)


def solve(t, sample_bits, table_bits):
    """the header's solver in Python floats (IEEE doubles), operation for operation -> (F0, f[0 .. n_hist-2], occupancy);
    None where the library refuses (the table is full, or the histogram does not sum to 2^table_bits)"""
    t = [int(x) for x in t]
    n_hist, R = len(t), 1 << table_bits
    if sum(t) != R or t[0] == 0:
        return None
    t0 = float(t[0])
    L = float(table_bits) * math.log(2.0) - math.log(t0)
    F0 = 0.0 if t[0] == R else math.ldexp(L, table_bits + sample_bits)
    phi, f = [0.0] * n_hist, [0.0] * (n_hist - 1)
    for i in range(1, n_hist - 1):
        v = 0.0
        if t[0] != R:
            s = 0.0
            for j in range(1, i):
                s += float(j) * float(t[i - j]) * phi[j]
            v = float(t[i]) / (t0 * L) - s / (float(i) * t0)
        phi[i] = v
        f[i] = abs(v) * F0
    return F0, np.array(f), 1.0 - t0 / float(R)


ACC_K, ACC_READS, ACC_LEN = 25, 4096, 100
_acc = {}


def accuracy_reads():
    """the reads of the accuracy input, back to back (read_len = ACC_LEN) -> uint8 array"""
    if "reads" not in _acc:
        rng = np.random.RandomState(20250)
        genome = rng.randint(0, 4, 20000)
        offs = rng.randint(0, genome.size - ACC_LEN + 1, ACC_READS)
        reads = genome[offs[:, None] + np.arange(ACC_LEN)[None, :]]
        sub = rng.random_sample(reads.shape) < 0.01
        reads = np.where(sub, (reads + rng.randint(1, 4, reads.shape)) % 4, reads)  # a substitution changes the base
        _acc["reads"] = np.frombuffer(b"ACGT", np.uint8)[reads].reshape(-1).copy()
    return _acc["reads"]


def accuracy_hashes(oracle):
    """(windows, hashes) of the accuracy input; computed once"""
    if "hashes" not in _acc:
        _acc["hashes"] = window_hashes(oracle, accuracy_reads(), ACC_K, read_len=ACC_LEN)
    return _acc["hashes"]


def accuracy_truth(oracle):
    """(distinct k-mers, those seen once) by np.unique over the canonical hashes"""
    _, counts = np.unique(accuracy_hashes(oracle)[1], return_counts=True)
    return counts.size, int((counts == 1).sum())
