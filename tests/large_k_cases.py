"""Inputs and expectations for the large-k tests (tests/test_gpu_large_k.py on the GPU; tests/test_oracle_vs_ref.py,
tests/test_oracle_golden.py and tests/golden/make_golden.py on the CPU).

Every input is built from a RECIPE -- a numpy RandomState seed, a length, an alphabet, a lowercase run and a list of
(position, byte) for the bytes put in afterwards -- so that tests/golden/large_k.json can pin the genuine reference's
outputs by their SHA-256 without storing the inputs.  Expected values come from the CPU oracle (oracle/btl_oracle.c),
which that file and test_oracle_vs_ref.py pin to the reference at these k."""
import ctypes as C
import hashlib

import numpy as np

GOLDEN_FILE = "large_k.json"
N, RAW_BYTES = ord("N"), (1, 3, 4, 5, 7)

# ---- thresholds derived on the host ------------------------------------------------------------------------------
K_BASE = [129, 1010, 1011, 2049, 4097, 32768]
PASS_A_BINS = [256, 512, 1024]


def tile_cap(tile_windows, k):
    """seq_tile_cap (csrc/internal.hpp): bytes of LDS of a tile image"""
    return (tile_windows + k - 1 + 30) // 16 * 16


def first_k_with_extra_staging(threads, windows_per_thread=8):
    """the smallest k at which seq_stage_convert's "large k only" loop runs: a thread converts windows_per_thread/4 + 1
    words of its own first, the loop takes the words of the image from (that many) * threads on"""
    ahead = (windows_per_thread // 4 + 1) * threads
    k = 1
    while tile_cap(threads * windows_per_thread, k) // 4 <= ahead:
        k += 1
    return k


def first_k_reading_the_extra_words(threads, mis=0, windows_per_thread=8):
    """the smallest k at which a window READS a base that loop staged (below it the loop converts slack only: the image
    is rounded up by up to 30 bytes): the last window of a tile starts at LDS byte tile - 1 + mis and ends k - 1 later"""
    ahead_bytes = (windows_per_thread // 4 + 1) * threads * 4
    return ahead_bytes - threads * windows_per_thread - mis + 2


def plan_pass_a(lib, k, h, bins):
    """btlbf_plan_pass_a -> (fits, dyn LDS, positional table, start bitmap words)"""
    out = (C.c_uint32 * 4)()
    assert lib.btlbf_plan_pass_a(k, h, bins, out) == 0
    return tuple(out)


def last_k(pred, lo=1, hi=32768):
    """the largest k in [lo, hi] with pred(k), for a predicate that holds up to some k and never after"""
    assert pred(lo)
    if pred(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def pass_a_boundaries(lib, h=3):
    """{bins: (last k pass A fits, last k it has room for the ragged layout's start bitmap)} from the library's planner"""
    out = {}
    for bins in PASS_A_BINS:
        # from k = 129 on: plain ntHash has no positional table to give way there (k <= 128 is the suite's old ground)
        fits = last_k(lambda k: plan_pass_a(lib, k, h, bins)[0] == 1, lo=129)
        ragged = last_k(lambda k: plan_pass_a(lib, k, h, bins)[3] != 0, lo=129)
        # monotone: checked on a coarse grid as well, so that the bisection's premise is not taken on trust
        grid = [plan_pass_a(lib, k, h, bins) for k in range(129, 32769, 97)]
        assert all(a[0] >= b[0] and bool(a[3]) >= bool(b[3]) for a, b in zip(grid, grid[1:]))
        out[bins] = (fits, ragged)
    return out


def k_ladder(lib):
    b = pass_a_boundaries(lib)
    ks = set(K_BASE)
    for fits, _ in b.values():
        ks.update((fits, fits + 1))
    return sorted(ks)


# ---- inputs from recipes -----------------------------------------------------------------------------------------
def build_input(rec):
    rng = np.random.RandomState(rec["seed"])
    s = rng.choice(list(rec["alphabet"].encode("latin-1")), rec["length"]).astype(np.uint8)
    lo, hi = rec["lower"]
    s[lo:hi] |= 0x20
    for p, b in rec["bytes"]:
        s[p] = b
    return s.tobytes()


def seq_recipe(seed, k, raw):
    """a sequence of 2k + 600 bases: a raw byte near the start, a lowercase run, an N with clean windows on either side"""
    return dict(seed=seed, length=2 * k + 600, alphabet="ACGT", lower=[200, 200 + k // 2], bytes=[[100, raw], [k + 300, N]])


def make_seeds(seed, k, n_seeds, p_one=0.7):
    """random spaced seeds whose first and last characters are 1"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_seeds):
        s = (rng.rand(k) < p_one).astype(np.uint8)
        s[0] = s[-1] = 1
        out.append("".join("01"[c] for c in s))
    return out


def kmer_recipe(seed, k, n=8):
    """n raw k-mers back to back: ACGT, one lowercase, one with U and u, one with an N in the middle, one with a raw byte,
    and one (k-mer 6) with an N among its last two bases: at k % 4 = 2 or 3 that indexes the reference's 2- / 3-base tail
    table out of range, so the k-mer has no value there (valid = 0); at k % 4 = 0 or 1 it has one"""
    mid = k // 2
    return dict(seed=seed, length=n * k, alphabet="ACGT", lower=[k, 2 * k],
                bytes=[[2 * k + 5, ord("U")], [2 * k + mid, ord("u")], [3 * k + mid, N], [4 * k + 7, 3], [7 * k - 2, N]])


def golden_cases():
    """the cases of tests/golden/large_k.json: (name, kind, parameters, input recipe)"""
    cases = []
    for i, k in enumerate([129, 257, 1010, 1011, 2049, 4097, 32768]):
        for h in (1, 3):
            cases.append(dict(name="nthash_k%d_h%d" % (k, h), kind="nthash", k=k, h=h,
                              input=seq_recipe(1000 + k + h, k, RAW_BYTES[i % 5])))
    for i, (k, n_seeds) in enumerate([(129, 2), (512, 3), (1024, 4)]):
        cases.append(dict(name="sthash_k%d" % k, kind="sthash", k=k, h2=1, seeds=dict(seed=2000 + k, n=n_seeds, p_one=0.7),
                          input=seq_recipe(3000 + k, k, RAW_BYTES[(i + 2) % 5])))
    for k in (1023, 1024, 4097, 32768):
        cases.append(dict(name="kmer_k%d" % k, kind="kmer", k=k, h=3, input=kmer_recipe(4000 + k, k)))
    return cases


def sha_u64(a):
    return hashlib.sha256(np.ascontiguousarray(a).astype("<u8").tobytes()).hexdigest()


def run_case(engine, case):
    """the outputs of one golden case from `engine` (the oracle or the reference: nthash_seq, sthash_seq, kmer_hashes)
    -> dict(n, pos, hashes[, strand]) of arrays; for raw k-mers `pos` are the indices of the k-mers the oracle calls
    defined and `engine` is asked about those alone"""
    s = build_input(case["input"])
    k = case["k"]
    if case["kind"] == "nthash":
        pos, hv = engine.nthash_seq(s, case["h"], k)
        return dict(pos=pos, hashes=hv)
    if case["kind"] == "sthash":
        sd = case["seeds"]
        pos, hv, st = engine.sthash_seq(s, make_seeds(sd["seed"], k, sd["n"], sd["p_one"]), case["h2"], k)
        return dict(pos=pos, hashes=hv, strand=st)
    raise ValueError(case["kind"])


def digest_case(out):
    d = dict(n=int(len(out["pos"])), pos=sha_u64(out["pos"]), hashes=sha_u64(out["hashes"]))
    if "strand" in out:
        d["strand"] = sha_u64(out["strand"])
    return d


def kmer_case_outputs(oracle, case, ref=None):
    """raw k-mers: the oracle's (hashes, defined); with `ref`, the reference's rows for the defined k-mers"""
    s = build_input(case["input"])
    k, h = case["k"], case["h"]
    hv, ok = oracle.kmer_hashes(s, k, h)
    idx = np.flatnonzero(ok)
    rows = hv[idx] if ref is None else np.array([ref.kmer_hashes(s[i * k:(i + 1) * k], k, h) for i in idx], np.uint64).reshape(-1, h)
    return dict(pos=idx, hashes=rows), hv, ok


# ---- buffers of the GPU tests ------------------------------------------------------------------------------------
class Buf:
    """a sequence buffer with its layout: bytes, the (lo, hi) of its sequences, starts / read_len"""

    def __init__(self, parts, kind):
        self.buf = b"".join(parts)
        self.n = len(self.buf)
        offs = np.cumsum([0] + [len(p) for p in parts])
        self.seqs = list(zip(offs[:-1].tolist(), offs[1:].tolist()))
        self.starts = offs.astype(np.uint64) if kind == "ragged" else None
        self.read_len = len(parts[0]) if kind == "uniform" else 0
        self.kind = kind

    def kw(self):
        return dict(starts=self.starts, read_len=self.read_len)


def acgt(rng, n):
    return rng.choice(list(b"ACGT"), n).astype(np.uint8)


def ragged_buffer(k, seed=0):
    """sequences of 0, k-1, k, k+1, k+2047, k+2048, k+2049 and 2k+100 bases, shuffled: the 2k+100 one with an N k-1
    bases before its end, the k+1 one lowercase, the k+2047 one with a raw byte; total length no multiple of 64"""
    rng = np.random.RandomState(7000 + k + seed)
    lens = [0, k - 1, k, k + 1, k + 2047, k + 2048, k + 2049, 2 * k + 100]
    parts = []
    for n in lens:
        s = acgt(rng, n)
        if n == k + 1:
            s |= 0x20
        if n == k + 2047:
            s[k // 2] = RAW_BYTES[k % 5]
        if n == 2 * k + 100:
            s[n - k] = N
        parts.append(s.tobytes())
    order = rng.permutation(len(parts))
    parts = [parts[i] for i in order]
    if sum(map(len, parts)) % 64 == 0:
        parts.append(acgt(rng, 7).tobytes())
    return Buf(parts, "ragged")


def uniform_buffer(k, L, seed=0):
    """reads of L bases (L = k or k + 1): a few hundred, a dozen at the largest k; some with an N, a raw byte, lowercase"""
    rng = np.random.RandomState(9000 + k + L + seed)
    n_reads = max(12, min(300, 300000 // L))
    if L % 64:  # (a read length that is a multiple of 64 leaves no choice)
        while (n_reads * L) % 64 == 0:
            n_reads += 1
    parts = []
    for i in range(n_reads):
        s = acgt(rng, L)
        if i % 7 == 3:
            s[rng.randint(L)] = N
        if i % 7 == 5:
            s[rng.randint(L)] = RAW_BYTES[i % 5]
        if i % 7 == 6:
            s |= 0x20
        parts.append(s.tobytes())
    return Buf(parts, "uniform")


class Windows:
    """per window of a buffer, from the oracle: clean, the hash row (zeros where not clean), the strand word"""

    def __init__(self, oracle, b, k, h, seeds=None):
        n = b.n
        self.clean = np.zeros(n, bool)
        self.rows = np.zeros((n, h), np.uint64)
        self.strand = np.zeros(n, np.uint64)
        for lo, hi in b.seqs:
            if hi - lo < k:
                continue
            if seeds:
                pos, hv, st = oracle.sthash_seq(b.buf[lo:hi], seeds, 1, k)
                word = (st.astype(np.uint64) << np.arange(h, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            else:
                pos, hv = oracle.nthash_seq(b.buf[lo:hi], h, k)
            p = pos.astype(np.int64) + lo
            self.clean[p] = True
            self.rows[p] = hv
            if seeds:
                self.strand[p] = word
        self.idx = np.flatnonzero(self.clean)
        self.crows = np.ascontiguousarray(self.rows[self.idx])
        self.windows = sum(max(hi - lo - k + 1, 0) for lo, hi in b.seqs)


def spread(n, idx, values, dtype=bool):
    out = np.zeros(n, dtype)
    out[idx] = values
    return out


def insert_and_check_expectation(body, bits, w, n):
    """(hit, ambiguous) per window of a parallel insertAndCheck (include/btlbf.h): 1 where all bits were set before the
    call, 0 where a clear bit is probed by no other window of the call, either answer for the rest"""
    m, h = w.crows.shape
    pos = (w.crows % np.uint64(bits)).astype(np.int64)
    before = ((body[pos >> 3] >> (pos & 7).astype(np.uint8)) & 1).astype(bool)
    pairs = np.unique(np.stack([pos.ravel(), np.repeat(np.arange(m), h)]), axis=1)
    upos, n_windows = np.unique(pairs[0], return_counts=True)
    alone = n_windows[np.searchsorted(upos, pos)] == 1
    one = before.all(axis=1)
    zero = (~before & alone).any(axis=1)
    return spread(n, w.idx, one), spread(n, w.idx, ~(one | zero))

