"""A numpy model of the reference's CountingBloomFilter<T> for T = uint16_t, uint32_t, uint64_t
(CountingBloomFilter.hpp:26-379): geometry, the serial incrementMin / incrementAll / minCount / contains /
insertAndCheck, popCount / filtered_popcount, the header text, and the parallel-order checkers of
tests/update_order_model.py restated with MAX = 2^bits - 1 as a parameter.  No GPU import.

tests/test_wide_counter_vs_ref.py pins this model to the genuine reference; tests/test_gpu_wide_counters.py checks the
HIP kernels against it.  The seeded cases both use are built here (CASES, make_case).
"""
import hashlib

import numpy as np
from update_order_model import ContractViolation, _none, _require, positions  # noqa: F401  (shared as they are)

DTYPES = {16: np.dtype("<u2"), 32: np.dtype("<u4"), 64: np.dtype("<u8")}
KINDS = {8: 1, 16: 2, 32: 3, 64: 4}  # BTLBF_COUNTING*


def max_of(bits):
    return (1 << bits) - 1


def round_bytes(size_in_bytes):
    """CountingBloomFilter.hpp:40-49"""
    r = size_in_bytes % 8
    return size_in_bytes if r == 0 else size_in_bytes + 8 - r


class WideCBF:
    """CountingBloomFilter<T>(sizeInBytes, hashNum, kmerSize, countThreshold); `c` holds the counters as Python-int
    friendly uint64 (values stay below 2^bits), body() gives the bytes of the reference's m_filter"""

    def __init__(self, bits, size_in_bytes, h, k, thr=0, body=None):
        self.bits, self.h, self.k, self.thr = bits, h, k, thr
        self.max = max_of(bits)
        self.size_bytes = round_bytes(size_in_bytes)
        self.size = self.size_bytes // (bits // 8)  # m_size = m_sizeInBytes / sizeof(T)
        self.bits_per_counter = 8  # CountingBloomFilter.hpp:109: whatever T is
        self.c = [0] * self.size
        if body is not None:
            self.upload(body)

    def upload(self, body):
        a = np.frombuffer(bytes(body), DTYPES[self.bits])
        assert a.size == self.size
        self.c = [int(x) for x in a]

    def body(self):
        return np.array(self.c, dtype=np.uint64).astype(DTYPES[self.bits]).tobytes()

    def counters(self):
        return np.array(self.c, dtype=np.uint64).astype(DTYPES[self.bits])

    def pos(self, row):
        return [int(x) % self.size for x in row]  # hash % m_size: the counter count, not the byte count

    def min_count(self, row):  # :53-64
        return min(self.c[p] for p in self.pos(row))

    def contains(self, row):  # :190-196
        return self.min_count(row) >= self.thr

    def increment_min(self, row):  # :135-162, one thread: the first pass always succeeds
        ps = self.pos(row)
        mn = min(self.c[p] for p in ps)
        if mn == self.max:  # minVal > newVal
            return
        for p in ps:  # __sync_bool_compare_and_swap(&m_filter[pos], minVal, newVal), position by position
            if self.c[p] == mn:
                self.c[p] = mn + 1

    def increment_all(self, row):  # :165-183
        for p in self.pos(row):
            if self.c[p] != self.max:
                self.c[p] += 1

    def insert_and_check(self, row):  # :206-214
        found = self.contains(row)
        self.increment_min(row)
        return found

    def pop_count(self):  # :217-228
        return sum(1 for v in self.c if v != 0)

    def filtered_popcount(self):  # :231-242
        return sum(1 for v in self.c if v >= self.thr)

    def header(self):
        """storeHeader (:344-368) as libstdc++'s unordered_map orders cpptoml's table (the pinned files decide)"""
        return ("[BTLCountingBloomFilter_v1]\n\tBloomFilterSize = %d\n\tHashNum = %d\n\tKmerSize = %d\n"
                "\tBloomFilterSizeInBytes = %d\n\tBitsPerCounter = %d\n[HeaderEnd]\n"
                % (self.size, self.h, self.k, self.size_bytes, self.bits_per_counter)).encode()

    def file_bytes(self):
        return self.header() + self.body()


# ---------------------------------------------------------------------------------------------------------------
# parallel order: tests/update_order_model.py's M1-M4 / C0-C1 with MAX for 255.  Arrays are Python-int exact: object
# arrays would be slow, uint64 compares are exact, and sums are taken in Python ints.
# ---------------------------------------------------------------------------------------------------------------
def check_increment_all(after, expect_after):
    after, expect_after = np.asarray(after, np.uint64), np.asarray(expect_after, np.uint64)
    _require(after.shape == expect_after.shape, "A1", "body of %d counters, expected %d", after.size, expect_after.size)
    _none(after != expect_after, "A1", "counter %d is %d, incrementAll gives %d", after, expect_after)


def saturating_add(before, add, mx):
    """before + add per counter, cut at `mx` -> uint64 array (exact for 64 bits too: the addend is cut to the room
    below `mx` before it is added)"""
    b = np.asarray(before, np.uint64)
    return b + np.minimum(np.asarray(add, np.uint64), np.uint64(mx) - b)


def increment_all_exact(before, pos, mx):
    """incrementAll of the windows `pos` on `before`, order-free: saturating + (number of probes) per counter"""
    return saturating_add(before, np.bincount(np.asarray(pos, np.int64).ravel(), minlength=len(before)), mx)


def check_increment_min(before, after, upper, pos, mx):
    """M1-M4 for counters of maximum `mx`.  `upper`: incrementAll of the same windows on a copy of `before`."""
    before, after, upper = (np.asarray(x, np.uint64) for x in (before, after, upper))
    pos = np.asarray(pos, np.int64)
    size = before.size
    mxu = np.uint64(mx)
    _require(after.size == size, "M1", "body of %d counters, expected %d", after.size, size)
    touched = np.zeros(size, bool)
    touched[pos.ravel()] = True
    _none(after < before, "M1", "counter %d decreased from %d to %d", before, after)
    _none((before == mxu) & (after != mxu), "M1", "counter %d was at the maximum and is %d", after)
    _none(~touched & (after != before), "M1", "counter %d is probed by no window and went from %d to %d", before, after)
    _none(after > upper, "M2", "counter %d is %d, above incrementAll's %d", after, upper)
    if pos.size == 0:
        return
    bmin = before[pos].min(axis=1)
    need = np.where(bmin == mxu, mxu, bmin + np.uint64(1))
    got = after[pos].min(axis=1)
    _none(got < need, "M3", "window %d: minimum %d after the call, at least %d required (minimum before + 1, or the maximum)",
          got, need)
    if int(upper[touched].max()) < mx:
        n, h = pos.shape
        grew = sum(int(x) for x in after) - sum(int(x) for x in before)
        _require(n <= grew <= h * n, "M4", "the counters grew by %d in all; %d windows of %d probes allow %d .. %d", grew,
                 n, h, n, h * n)


def check_counting_insert_and_check(before, after, upper, pos, out, thr, mx):
    b, u = np.asarray(before, np.uint64), np.asarray(upper, np.uint64)
    pos = np.asarray(pos, np.int64)
    out = np.asarray(out).astype(np.uint8)
    _require(len(out) == len(pos), "C1", "%d reports for %d windows", len(out), len(pos))
    if len(out):
        t = np.uint64(thr)
        _none((b[pos].min(axis=1) >= t) & (out != 1), "C1",
              "window %d reports %d although its minimum was >= %d before the call", out, thr)
        _none((u[pos].min(axis=1) < t) & (out != 0), "C0",
              "window %d reports %d although even incrementAll leaves its minimum < %d", out, thr)
    check_increment_min(before, after, upper, pos, mx)


# ---------------------------------------------------------------------------------------------------------------
# the seeded cases (the smallest shapes at which an implementation can still go wrong)
# ---------------------------------------------------------------------------------------------------------------
def prefill_values(bits):
    mx = max_of(bits)
    return (0, 1, 0xff, 0x100, mx - 2, mx - 1, mx)


def prefilled_body(bits, n_counters, seed):
    """counters drawn from {0, 1, 0xff, 0x100, MAX-2, MAX-1, MAX}: a 255 -> 256 carry inside the counter, saturation,
    and (16 bits) a counter at 0xffff beside one that is incremented"""
    rng = np.random.RandomState(seed)
    vals = prefill_values(bits)
    idx = rng.randint(0, len(vals), n_counters)
    return np.array([vals[i] for i in idx], dtype=np.uint64).astype(DTYPES[bits]).tobytes()


def reads_of(seed, k):
    """a few reads with repeated k-mers, one N and a read shorter than k -> [bytes]"""
    rng = np.random.RandomState(1000 + seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    r0 = acgt[rng.randint(0, 4, k + 40)].tobytes()
    r2 = bytearray(acgt[rng.randint(0, 4, k + 30)].tobytes())
    r2[k + 3] = ord("N")
    return [r0, r0[7:k + 33], bytes(r2), r0[: k - 1], r0, acgt[rng.randint(0, 4, k + 12)].tobytes()]


# name -> (sizeInBytes, h, k, threshold, ops, prefilled, widths, commit the stored file as a fixture)
SHAPES = {
    "c8": (8, 2, 8, 2, ("min", "all", "check"), True, (16, 32, 64), True),
    "c1000": (1000, 3, 25, 2, ("min", "all", "check"), True, (16, 32, 64), True),
    "c1000z": (1000, 3, 25, 1, ("min", "all"), False, (16, 32, 64), False),
    "c1000h1": (1000, 1, 25, 1, ("min",), True, (16, 32, 64), False),
    "c1000h5": (1000, 5, 25, 1, ("min", "all"), True, (16, 32, 64), False),
    "c4096": (4096, 3, 25, 1, ("min", "all"), True, (16, 32, 64), False),
    "unit": (100001, 5, 8, 1, ("min",), False, (16, 64), False),  # Tests/Unit/CountingBloomFilterTests.cpp's shape
}
CASES = [(shape, bits, op) for shape, v in SHAPES.items() for bits in v[6] for op in v[4]]
# seeds of the inputs, chosen on the CPU so that the REFERENCE's output meets the conditions of
# tests/test_wide_counter_vs_ref.py (its docstring lists them)
SEEDS = {"c8": 36, "c1000": 0, "c1000z": 0, "c1000h1": 0, "c1000h5": 0, "c4096": 0, "unit": 0}


def case_key(shape, bits, op):
    return "%s_u%d_%s" % (shape, bits, op)


def fixture_name(shape, bits, op):
    return "wcbf_%s_u%d_%s.bf" % (shape, bits, op)


def make_case(shape, bits):
    """-> (sizeInBytes, h, k, threshold, reads, body before the call as bytes)"""
    nbytes, h, k, thr, _, prefilled, _, _ = SHAPES[shape]
    seed = SEEDS[shape]
    n = round_bytes(nbytes) // (bits // 8)
    body = prefilled_body(bits, n, seed) if prefilled else bytes(round_bytes(nbytes))
    return nbytes, h, k, thr, reads_of(seed, k), body


def run_model(oracle, shape, bits, op):
    """the serial order over every clean window of every read -> (WideCBF after, out bits of insertAndCheck, rows)"""
    nbytes, h, k, thr, reads, body = make_case(shape, bits)
    f = WideCBF(bits, nbytes, h, k, thr, body)
    out, rows = [], []
    for s in reads:
        for row in oracle.nthash_seq(s, h, k)[1]:
            rows.append(row)
            if op == "min":
                f.increment_min(row)
            elif op == "all":
                f.increment_all(row)
            else:
                out.append(int(f.insert_and_check(row)))
    return f, out, np.array(rows, dtype=np.uint64).reshape(-1, h)


def figures(bits, before, after, rows, size, size_bytes):
    """what the conditions are asserted on: [counters > 255 after, counters saturated BY the call, 32-bit words with
    both 16-bit halves changed (0 for other widths), probes whose % counters and % bytes positions differ]"""
    b = np.frombuffer(before, DTYPES[bits]).astype(np.uint64)
    a = np.frombuffer(after, DTYPES[bits]).astype(np.uint64)
    mx = np.uint64(max_of(bits))
    ch = a != b
    both = int((ch[0::2] & ch[1::2]).sum()) if bits == 16 else 0
    differ = sum(1 for r in rows for v in r if int(v) % size != int(v) % size_bytes)
    return [int((a > np.uint64(255)).sum()), int(((a == mx) & (b != mx)).sum()), both, int(differ)]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()
