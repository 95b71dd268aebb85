"""The C ABI's output contract (include/btlbf.h, "output buffers"): a call stores EVERY byte of every output it is given
-- the caller need not initialise one -- and nothing outside [out, out + size).

Every other test reaches the library through engine._out, which hands it zeroed buffers, so a byte a route never writes
reads back as the right zero and a store past an output is never looked at.  Here the outputs are dirty and guarded
(tests/poison.py): each case runs under the poisons 0xFF and 0xA5, compares every byte of every output with an
expectation built as WHOLE arrays (bitmaps in full words, the positions >= len zero; rows and bytes of unclean windows
zero), and ends with check_guards().  Bit-exact, no tolerances.

  (a) the direct kernels, DEVICE and HOST, at the sizes where a tile, a word or a read ends -- against the CPU oracle
  (b) the forced partitioned query and (c) the two AUTO split routes -- against the direct kernel's answer obtained with
      the engine's zeroed outputs (what the suite pins to the oracle at these sizes), the route read from the profile
  (d) hash rows, raw k-mers, rank queries and per-sequence counts through raw ctypes -- against the oracle / numpy
  (e) miBF query, classify and classifyPairs -- against tests/mibf_model.py and tests/mibf_classify_model.py

HOST mode: the device staging of a host call comes from a pool (or the calling thread's mailbox) and holds what the
previous call left; it cannot be poisoned from outside.  Each HOST case in (a) is therefore preceded by a priming call
of the same sizes whose outputs are dense (the same layout, every read inserted, no N), which makes stale content in
the staging likely, not certain.  DEVICE mode is where the poison is deterministic.

A fixed read_len layout takes whole reads only (len % read_len != 0 is EINVAL, test_partial_trailing_read_is_einval),
so the uniform layouts here get len % 64 outside {0, 56..63} from their read count, not from a partial last read."""
import ctypes as C

import numpy as np
import pytest

import mibf_model as mm
from poison import POISONS, assert_bitmap, assert_same, check_guards, full_bitmap, host_bytes, poisoned_outputs
from test_gpu_auto_query import _assert_path, _np, bf, splice  # noqa: F401  (bf: fixture)
from test_gpu_parity import rand_seq

pytestmark = pytest.mark.gpu

C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]
BITS, K, H = 1 << 20, 31, 4           # the bit filter of (a) and (d)
CSIZE, CK, CH, THR = 1 << 20, 25, 3, 2  # the counting filter
MEMS = ["device", "host"]


def to_dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the source may be a read-only view of bytes)


def sync():
    import torch

    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# (a) layouts and whole-buffer expectations from the oracle
# ---------------------------------------------------------------------------------------------
class Layout:
    """reads under test (rand_seq: with N and other unclean bytes), priming reads of the same lengths (ACGT only), and
    which byte strings are in the filters: every priming read, and half of the material under test"""

    def __init__(self, rng, name, lens, kind):
        self.name, self.kind = name, kind
        test = [rand_seq(rng, n, 0.02) for n in lens]
        prime = [rng.choice(list(b"ACGT"), n).astype(np.uint8).tobytes() for n in lens]
        self.buf, self.prime = b"".join(test), b"".join(prime)
        self.n = len(self.buf)
        offs = np.cumsum([0] + list(lens))
        self.seqs = list(zip(offs[:-1].tolist(), offs[1:].tolist()))
        self.starts = offs.astype(np.uint64) if kind == "ragged" else None
        self.read_len = lens[0] if kind == "uniform" else 0
        if kind == "single":  # the first half of a long sequence; every other short one whole
            n = lens[0]
            self.inserted = [test[0][: n // 2]] if n >= 100 else [test[0]] * (n % 2)
        else:
            self.inserted = test[::2]
        self.primes = prime

    def args(self, mem, prime=False):
        """(seq, keywords of the layout) in host or device memory"""
        a = np.frombuffer(self.prime if prime else self.buf, np.uint8)
        st = self.starts
        if mem == "device":
            a, st = to_dev(a), None if st is None else to_dev(st.astype(np.int64))
        return a, dict(starts=st, read_len=self.read_len)


def uniform_count(L, at_least):
    """reads of L bytes, at least at_least bytes, with len % 64 in 1..55: the last bitmap word has a tail of 9 bits or
    more, and it is not the byte-granular tail a tile's last byte store would cover by accident"""
    n = -(-at_least // L)
    while not 1 <= (n * L) % 64 <= 55:
        n += 1
    return n


def make_layouts():
    rng = np.random.RandomState(2024)
    out = [Layout(rng, "single_%d" % n, [n], "single")
           for n in (1, CK - 1, CK, K - 1, K, 63, 64, 65, 100, 2047, 2048, 2049, 4100)]
    out += [Layout(rng, "uniform_%d" % L, [L] * uniform_count(L, 2100), "uniform") for L in (7, 31, 100, 150)]
    # beyond the 65536 bytes a host call takes through the mailbox: the staged path with a fixed read length
    out.append(Layout(rng, "uniform_150_staged", [150] * uniform_count(150, 65537), "uniform"))
    out.append(Layout(rng, "ragged", [0, 5, 30, 31, 32, 150, 150, 1, 2047, 2048, 4100, 0, 77, 31, 24, 25, 0, 0], "ragged"))
    return out


class Windows:
    """per window of a buffer: clean, the hash row (zeros where not clean), the strand word (spaced seeds)"""

    def __init__(self, oracle, buf, seqs, k, h, seeds=None):
        n = len(buf)
        self.clean = np.zeros(n, bool)
        self.rows = np.zeros((n, h), np.uint64)
        self.strand = np.zeros(n, np.uint64)
        for lo, hi in seqs:
            if hi == lo:
                continue
            if seeds:
                pos, hv, st = oracle.sthash_seq(buf[lo:hi], seeds, 1, k)
                word = (st.astype(np.uint64) << np.arange(h, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            else:
                pos, hv = oracle.nthash_seq(buf[lo:hi], h, k)
            p = pos.astype(np.int64) + lo
            self.clean[p] = True
            self.rows[p] = hv
            if seeds:
                self.strand[p] = word
        self.idx = np.flatnonzero(self.clean)
        self.crows = np.ascontiguousarray(self.rows[self.idx])


def spread(n, idx, values, dtype=bool):
    out = np.zeros(n, dtype)
    out[idx] = values
    return out


class Direct:
    """the two filters of (a) -- bodies built by the oracle and uploaded --, and the expectations of every layout"""

    def __init__(self, bf, oracle):
        self.bf, self.oracle = bf, oracle
        self.layouts = make_layouts()
        self.body = np.zeros(BITS // 8, np.uint8)
        self.cbf = bf.CountingBloomFilter(CSIZE, CH, CK, THR)
        self.cbody = np.zeros(self.cbf.size(), np.uint8)
        for lay in self.layouts:
            # counters: the priming reads twice (every window at the threshold), the reads under test once or twice
            for s, times in [(s, 2) for s in lay.primes] + [(s, 1 + i % 2) for i, s in enumerate(lay.inserted)]:
                if not s:
                    continue
                oracle.bf_insert_seq(self.body, BITS, H, K, s)
                _, hv = oracle.nthash_seq(s, CH, CK)
                for _ in range(times):
                    oracle.cbf_increment_min(self.cbody, CH, hv)
        self.flt = self.bit_filter()
        self.cbf.upload(self.cbody)
        self._win = {}

    def bit_filter(self):
        f = self.bf.BloomFilter(BITS, H, K)
        f.upload(self.body)
        return f

    def win(self, lay, k, h, seeds=None, prime=False):
        key = (lay.name, k, h, bool(seeds), prime)
        if key not in self._win:
            self._win[key] = Windows(self.oracle, lay.prime if prime else lay.buf, lay.seqs, k, h, seeds)
        return self._win[key]


@pytest.fixture(scope="module")
def direct(bf, oracle):
    return Direct(bf, oracle)


def check_query(name, got, n, clean, hit, want_valid, want_counts):
    ghit, gvalid, gcnt = got
    assert_bitmap(name + " hit_bits", ghit, hit, n)
    if want_valid:
        assert_bitmap(name + " valid_bits", gvalid, clean, n)
    else:
        assert gvalid is None
    if want_counts:
        assert_same(name + " counts", gcnt, np.array([clean.sum(), hit.sum()], np.uint64))
    else:
        assert gcnt is None


SHAPES = [(True, True), (False, False)]  # (valid bitmap, counts)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_contains_seqs_bit_filter(direct, monkeypatch, byte, mem):
    poisoned_outputs(monkeypatch, byte)
    n_hit = n_miss = 0
    for lay in direct.layouts:
        w = direct.win(lay, K, H)
        hit = spread(lay.n, w.idx, direct.oracle.bf_contains(direct.body, BITS, H, w.crows).astype(bool))
        for wv, wc in SHAPES:
            if mem == "host":
                seq, kw = lay.args(mem, prime=True)
                direct.flt.containsSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            seq, kw = lay.args(mem)
            got = direct.flt.containsSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            check_query("%s/%s containsSeqs" % (lay.name, mem), got, lay.n, w.clean, hit, wv, wc)
        n_hit += int(hit.sum())
        n_miss += int((w.clean & ~hit).sum())
    assert n_hit > 5000 and n_miss > 5000
    check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_contains_and_min_count_seqs_counting_filter(direct, monkeypatch, byte, mem):
    """containsSeqs (minimum >= threshold) and minCountSeqs: all len bytes of min_out, 0 where not clean"""
    poisoned_outputs(monkeypatch, byte)
    seen = set()
    for lay in direct.layouts:
        w = direct.win(lay, CK, CH)
        mn, ct = direct.oracle.cbf_query(direct.cbody, CH, THR, w.crows)
        hit = spread(lay.n, w.idx, ct.astype(bool))
        want_min = spread(lay.n, w.idx, mn, np.uint8)
        seen |= set(mn.tolist())
        for wv, wc in SHAPES:
            if mem == "host":
                seq, kw = lay.args(mem, prime=True)
                direct.cbf.containsSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            seq, kw = lay.args(mem)
            got = direct.cbf.containsSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            check_query("%s/%s counting containsSeqs" % (lay.name, mem), got, lay.n, w.clean, hit, wv, wc)
        if mem == "host":
            seq, kw = lay.args(mem, prime=True)
            direct.cbf.minCountSeqs(seq, **kw)
        seq, kw = lay.args(mem)
        gmin, gvalid = direct.cbf.minCountSeqs(seq, **kw)
        assert_same("%s/%s min_out" % (lay.name, mem), gmin, want_min)
        assert_bitmap("%s/%s minCountSeqs valid_bits" % (lay.name, mem), gvalid, w.clean, lay.n)
    assert {0, 1, 2} <= seen
    check_guards()


def insert_and_check_expectation(body, w, n):
    """(hit, ambiguous) per window.  The call runs its windows in parallel order (btlbf.h): a clean window whose h bits
    were all set before the call reports 1; one with a clear bit that no OTHER window of the call probes reports 0;
    what is left -- every clear bit shared with another window -- may report either, and is the only thing not compared"""
    m = len(w.idx)
    pos = (w.crows % np.uint64(BITS)).astype(np.int64)
    before = np.unpackbits(body, bitorder="little")[pos].astype(bool)
    pairs = np.unique(np.stack([pos.ravel(), np.repeat(np.arange(m), H)]), axis=1)  # (position, window), distinct
    upos, n_windows = np.unique(pairs[0], return_counts=True)
    alone = n_windows[np.searchsorted(upos, pos)] == 1
    one = before.all(axis=1)
    zero = (~before & alone).any(axis=1)
    return spread(n, w.idx, one), spread(n, w.idx, ~(one | zero))


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_insert_and_check_seqs(direct, monkeypatch, byte, mem):
    """a fresh copy of the filter per call (the call inserts); the filter afterwards is the oracle's insert"""
    poisoned_outputs(monkeypatch, byte)
    n_amb = n_zero = 0
    for lay in direct.layouts:
        w = direct.win(lay, K, H)
        hit, amb = insert_and_check_expectation(direct.body, w, lay.n)
        after = direct.body.copy()
        direct.oracle.bf_insert(after, BITS, H, w.crows)
        for wv, wc in SHAPES:
            if mem == "host":
                seq, kw = lay.args(mem, prime=True)
                direct.bit_filter().insertAndCheckSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            f = direct.bit_filter()
            seq, kw = lay.args(mem)
            got = f.insertAndCheckSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            name = "%s/%s insertAndCheckSeqs" % (lay.name, mem)
            got_bits = np.unpackbits(host_bytes(got[0]), bitorder="little")[: lay.n].astype(bool)
            want = np.where(amb, got_bits, hit)  # (the tail of the last word is never ambiguous: assert_bitmap has it)
            check_query(name, got, lay.n, w.clean, want, wv, wc)
            assert (f.download() == after).all(), name
        n_amb += int(amb.sum())
        n_zero += int((w.clean & ~hit & ~amb).sum())
    assert n_amb * 20 < n_zero  # nearly every answer is determined
    check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_hash_seqs(direct, monkeypatch, byte, mem):
    """every row: zeros for unclean windows and for the windows past len - k; the valid bitmap in whole words"""
    poisoned_outputs(monkeypatch, byte)
    for lay in direct.layouts:
        w = direct.win(lay, K, H)
        if mem == "host":
            seq, kw = lay.args(mem, prime=True)
            direct.bf.hash_seqs(seq, H, K, **kw)
        seq, kw = lay.args(mem)
        hv, valid = direct.bf.hash_seqs(seq, H, K, **kw)
        assert_same("%s/%s hash_seqs hashes" % (lay.name, mem), hv, w.rows)
        assert_bitmap("%s/%s hash_seqs valid_bits" % (lay.name, mem), valid, w.clean, lay.n)
    check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_sthash_seqs(direct, monkeypatch, byte, mem):
    """spaced seeds: rows, valid bitmap and every strand word (0 for unclean windows)"""
    poisoned_outputs(monkeypatch, byte)
    for lay in direct.layouts:
        w = direct.win(lay, K, H, C5_SEEDS)
        if mem == "host":
            seq, kw = lay.args(mem, prime=True)
            direct.bf.sthash_seqs(seq, C5_SEEDS, 1, K, **kw)
        seq, kw = lay.args(mem)
        hv, valid, st = direct.bf.sthash_seqs(seq, C5_SEEDS, 1, K, **kw)
        assert_same("%s/%s sthash_seqs hashes" % (lay.name, mem), hv, w.rows)
        assert_bitmap("%s/%s sthash_seqs valid_bits" % (lay.name, mem), valid, w.clean, lay.n)
        assert_same("%s/%s sthash_seqs strand_bits" % (lay.name, mem), st, w.strand)
    assert any(direct.win(lay, K, H, C5_SEEDS).strand.any() for lay in direct.layouts)
    check_guards()


@pytest.mark.parametrize("mem", MEMS)
def test_partial_trailing_read_is_einval(direct, monkeypatch, mem):
    """len % read_len != 0: refused before anything is launched -- the guards stand"""
    poisoned_outputs(monkeypatch, 0xA5)
    lay = next(x for x in direct.layouts if x.name == "uniform_100")
    seq, kw = lay.args(mem)
    with pytest.raises(direct.bf._lib.BtlbfError) as ei:
        direct.flt.containsSeqs(seq[:-3], read_len=100, want_valid=True, want_counts=True)
    assert ei.value.code == direct.bf._lib.EINVAL
    check_guards()


# ---------------------------------------------------------------------------------------------
# (b) forced partitioned query, (c) AUTO split routes: against the direct kernel's answer
# ---------------------------------------------------------------------------------------------
PK, PH = 31, 4


def counts_only(flt, q, kw):
    """contains() with neither bitmap (the C++ shim's countReads) -> the counts output"""
    from btl_bloomfilter_amd import engine as e

    b = e._Buf(q)
    lay, keep = e._layout(kw.get("starts"), kw.get("read_len", 0), b.mem)
    cnt, p_cnt = e._out(b, 2, np.uint64)
    e.check(flt._L.btlbf_contains_seqs(flt._h, b.ptr, b.nbytes, C.byref(lay) if lay else None, None, None, p_cnt, b.mem,
                                       e._stream_ptr(None, b.keep)))
    return cnt


def three_call_shapes(flt, q, kw, mode, monkeypatch, byte, check_route):
    """`mode` under poison, in the three call shapes, every output word against the direct kernel's answer into the
    engine's zeroed outputs plus the rule that positions >= len are 0; check_route(profile, call index) per call"""
    n = q.numel()
    flt.setQueryMode("direct")
    hit_d, valid_d, cnt_d = (_np(x) for x in flt.containsSeqs(q, want_valid=True, want_counts=True, **kw))
    hit_b = np.unpackbits(hit_d.view(np.uint8), bitorder="little").astype(bool)
    valid_b = np.unpackbits(valid_d.view(np.uint8), bitorder="little").astype(bool)
    assert not hit_b[n:].any() and not valid_b[n:].any() and not (hit_b & ~valid_b).any()
    hit_b, valid_b = hit_b[:n], valid_b[:n]
    assert cnt_d.tolist() == [int(valid_b.sum()), int(hit_b.sum())] and 0 < cnt_d[1] < cnt_d[0]
    want_cnt = np.array([valid_b.sum(), hit_b.sum()], np.uint64)
    flt.setQueryMode(mode)
    flt.setProfiling(True)
    poisoned_outputs(monkeypatch, byte)
    profs = []
    try:
        flt.getProfile()
        hit_1, valid_1, cnt_1 = flt.containsSeqs(q, want_valid=True, want_counts=True, **kw)
        sync()
        profs.append(flt.getProfile())
        hit_2, none_2, cnt_2 = flt.containsSeqs(q, want_valid=False, want_counts=True, **kw)
        sync()
        profs.append(flt.getProfile())
        cnt_3 = counts_only(flt, q, kw)
        sync()
        profs.append(flt.getProfile())
    finally:
        flt.setProfiling(False)
        flt.setQueryMode("auto")
    print(mode, [{name: v[1] for name, v in p.items()} for p in profs], cnt_d.tolist())
    assert_bitmap("with valid: hit_bits", hit_1, hit_b, n)
    assert_bitmap("with valid: valid_bits", valid_1, valid_b, n)
    assert_same("with valid: counts", cnt_1, want_cnt)
    assert_bitmap("without valid: hit_bits", hit_2, hit_b, n)
    assert none_2 is None
    assert_same("without valid: counts", cnt_2, want_cnt)
    assert_same("counts only: counts", cnt_3, want_cnt)
    check_guards()
    for i, prof in enumerate(profs):
        check_route(prof, i)


@pytest.fixture(scope="module")
def big(bf):
    """get(bits, n_reads, L, budget) -> (filter with the reads of seed 42 inserted, the reads), made once"""
    made = {}

    def get(bits, n, L, budget=None):
        key = (bits, n, L, budget)
        if key not in made:
            reads = bf.synth_reads_device(42, 0, n, L)
            flt = bf.BloomFilter(bits, PH, PK)
            flt.insertSeqs(reads, read_len=L)
            if budget:
                flt.setInsertMode(*budget)
            made[key] = (flt, reads)
        return made[key]

    return get


def partitioned_ran(min_batches):
    """min_batches 0: the budget holds no plan, the partitioned query declines before its first launch and the direct
    kernel answers (tests/test_gpu_query_fallbacks.py) -- also into dirty outputs"""
    def check(prof, i):
        c = {name: v[1] for name, v in prof.items()}
        if min_batches == 0:
            assert c == {"query_direct": 1}, (i, prof)
            return
        # pass A once per batch and the test pass per batch and group: the pipeline ran, it did not decline
        assert c.get("query_hash", 0) >= min_batches and c.get("query_test", 0) >= c.get("query_hash", 0), (i, prof)
        assert c.get("other", 0) == 0, (i, prof)
    return check


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("case,bits,miss_reads,n,L,ragged,budget,min_batches", [
    ("few_misses", 1 << 30, 3, 40000, 150, False, None, 1),
    ("fail_list_overflow", 1 << 30, 39000, 40000, 150, False, None, 1),
    ("modulo_filter", 3 << 22, 50, 40000, 150, False, None, 1),
    ("tail_22_bits", 1 << 30, 3, 40001, 150, False, None, 1),       # len % 64 == 22: the last tile writes the tail
    # 590 whole tiles of pass A's read grid (68 reads each) and len % 64 == 16: the last tile is full, and the six zero
    # bytes up to the end of the last bitmap word lie beyond its own bytes
    ("full_last_tile", 1 << 30, 3, 40120, 150, False, None, 1),
    ("odd_read_len", 1 << 30, 3, 40000, 151, False, None, 1),
    ("no_read_grid", 1 << 30, 3, 5455, 1100, False, None, 1),       # per-lane bitmaps; len % 64 == 52
    ("ragged", 1 << 30, 3, 40000, 150, True, None, 1),
    # a scratch budget: 48 MiB hold no plan for this filter (the call declines to the direct kernel); 72 MiB give four
    # batches and 96 MiB three, whose pass-A tiles do not end on the resolve kernel's tiles: its &= meets the seams
    ("budget_48m_declines", 1 << 30, 3, 40000, 150, False, ("partitioned", 48 << 20), 0),
    ("budget_72m_batches", 1 << 30, 3, 40000, 150, False, ("partitioned", 72 << 20), 2),
    ("budget_96m_batches", 1 << 30, 3, 40000, 150, False, ("partitioned", 96 << 20), 2),
])
def test_forced_partitioned_query(bf, big, monkeypatch, byte, case, bits, miss_reads, n, L, ragged, budget, min_batches):
    import torch

    flt, reads = big(bits, n, L, budget)
    q = reads.clone()
    idx = torch.arange(miss_reads, device="cuda") * (n // miss_reads)
    q.view(n, L)[idx] = bf.synth_reads_device(43, 0, miss_reads, L).view(miss_reads, L)
    q[12345] = ord("N")
    if case == "tail_22_bits":
        assert q.numel() % 64 == 22
    grid = (C.c_uint32 * 4)()
    bf._lib.check(bf._lib.load().btlbf_plan_read_grid(PK, PH, L, 512, grid))
    if case == "no_read_grid":
        assert not any(grid), list(grid)
    if case == "full_last_tile":
        assert grid[0] and n % grid[0] == 0 and q.numel() % 64 == 16 and (q.numel() + 63) // 64 * 8 - q.numel() // 8 == 6
    kw = dict(starts=torch.arange(n + 1, device="cuda", dtype=torch.int64) * L) if ragged else dict(read_len=L)
    three_call_shapes(flt, q, kw, "partitioned", monkeypatch, byte, partitioned_ran(min_batches))


@pytest.fixture(scope="module")
def split_filter(bf):
    """the filter and reads of tests/test_gpu_query_fallbacks.py with a budget the plans fit (256 MiB: below 2 GiB, so
    the short fail list of part_tail and its few_cold of 137 reads apply); 40001 reads, of which 40000 are inserted"""
    bits, L, n = 1 << 30, 150, 40000
    reads = bf.synth_reads_device(42, 0, n + 1, L)
    flt = bf.BloomFilter(bits, PH, PK)
    flt.insertSeqs(reads[: n * L], read_len=L)
    flt.setInsertMode("auto", scratch_bytes=256 << 20)
    return flt, reads, n, L


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("route,n_extra", [("split_cold", 0), ("split_warm", 0), ("split_cold", 1)])
def test_auto_split_routes(bf, split_filter, monkeypatch, byte, route, n_extra):
    """SplitCold: every 10th read foreign (the cold reads' answers ORed into the caller's bitmaps, counts[1] the
    popcount of the whole finished bitmap); SplitWarm: a third foreign (both bitmaps merged from compacted ones);
    SplitCold again with 40001 reads: len % 64 == 22"""
    flt, reads, n, L = split_filter
    n += n_extra
    foreign = np.arange(0, n, 10) if route == "split_cold" else np.arange(n // 3) * 3 + 1
    q = splice(bf, reads[: n * L].clone(), n, L, foreign)
    assert (q.numel() % 64 != 0) == bool(n_extra)

    def check(prof, i):  # (the counts-only call of SplitWarm has no bitmaps to merge)
        _assert_path(prof, route, 1, False, merges=not (route == "split_warm" and i == 2))

    three_call_shapes(flt, q, dict(read_len=L), "auto", monkeypatch, byte, check)


# ---------------------------------------------------------------------------------------------
# (d) hash rows, raw k-mers, rank, per-sequence counts: raw ctypes
# ---------------------------------------------------------------------------------------------
ROW_NS = [1, 63, 64, 65, 1000]


def raw_in(a, mem):
    """an input array for a raw call -> (keep-alive, c_void_p, BTLBF_HOST / DEVICE, stream, torch device or None)"""
    from btl_bloomfilter_amd import engine as e

    if mem == "device":
        t = to_dev(a.view(np.int64) if a.dtype == np.uint64 else a)
        return t, C.c_void_p(t.data_ptr()), e.DEVICE, e._stream_ptr(None, t), t.device
    a = np.ascontiguousarray(a)
    return a, C.c_void_p(a.ctypes.data), e.HOST, None, None


def probe_rows(direct, rng, n, k, h):
    """n hash rows: about half of them rows of k-mers that are in the filters, the rest random"""
    known = np.concatenate([direct.oracle.nthash_seq(lay.prime, h, k)[1] for lay in direct.layouts[8:12]])
    rows = rng.randint(0, 2**63, size=(n, h)).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, (n, h)).astype(np.uint64)
    take = rng.rand(n) < 0.5
    rows[take] = known[rng.randint(0, len(known), int(take.sum()))]
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_hash_row_calls(direct, monkeypatch, byte, mem):
    """btlbf_contains_hashes, btlbf_min_count_hashes, btlbf_insert_and_check_hashes (serial order: the oracle's loop):
    each of the n bytes"""
    reg = poisoned_outputs(monkeypatch, byte)
    L, lib, o = direct.bf._lib.load(), direct.bf._lib, direct.oracle
    rng = np.random.RandomState(77)
    ones = 0
    for n in ROW_NS:
        rows = probe_rows(direct, rng, n, K, H)
        keep, p_rows, memc, stream, dev = raw_in(rows, mem)
        out, p_out = reg.alloc(n, np.uint8, dev, "contains_hashes n=%d" % n)
        lib.check(L.btlbf_contains_hashes(direct.flt._h, p_rows, n, p_out, memc, stream))
        want = o.bf_contains(direct.body, BITS, H, rows)
        assert_same("contains_hashes n=%d" % n, out, want)
        ones += int(want.sum())

        f, mine = direct.bit_filter(), direct.body.copy()
        out, p_out = reg.alloc(n, np.uint8, dev, "insert_and_check_hashes n=%d" % n)
        lib.check(L.btlbf_insert_and_check_hashes(f._h, p_rows, n, p_out, lib.ORDER_SERIAL, memc, stream))
        assert_same("insert_and_check_hashes n=%d" % n, out, o.bf_insert_and_check(mine, BITS, H, rows))
        assert (f.download() == mine).all()

        crows = probe_rows(direct, rng, n, CK, CH)
        keep2, p_rows, memc, stream, dev = raw_in(crows, mem)
        mn, ct = o.cbf_query(direct.cbody, CH, THR, crows)
        out, p_out = reg.alloc(n, np.uint8, dev, "min_count_hashes n=%d" % n)
        lib.check(L.btlbf_min_count_hashes(direct.cbf._h, p_rows, n, p_out, memc, stream))
        assert_same("min_count_hashes n=%d" % n, out, mn)
        out, p_out = reg.alloc(n, np.uint8, dev, "counting contains_hashes n=%d" % n)
        lib.check(L.btlbf_contains_hashes(direct.cbf._h, p_rows, n, p_out, memc, stream))
        assert_same("counting contains_hashes n=%d" % n, out, ct)
    assert ones > 300
    reg.check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_rank_query(direct, monkeypatch, byte, mem):
    """btlbf_rank_query: both outputs, for positions and for hash values"""
    reg = poisoned_outputs(monkeypatch, byte)
    L, lib = direct.bf._lib.load(), direct.bf._lib
    rs = direct.bf.RankSupport(direct.flt)
    bits = np.unpackbits(direct.body, bitorder="little")
    csum = np.zeros(BITS + 1, np.uint64)  # csum[p] = set bits before p
    csum[1:] = np.cumsum(bits, dtype=np.uint64)
    rng = np.random.RandomState(5)
    for n in ROW_NS:
        for hashes in (0, 1):
            v = rng.randint(0, 2**63, n).astype(np.uint64) if hashes else rng.randint(0, BITS, n).astype(np.uint64)
            if not hashes:
                v[0], v[-1] = BITS - 1, 0
            keep, p_v, memc, stream, dev = raw_in(v, mem)
            rank, p_rank = reg.alloc(n, np.uint64, dev, "rank_out n=%d" % n)
            bit, p_bit = reg.alloc(n, np.uint8, dev, "bit_out n=%d" % n)
            lib.check(L.btlbf_rank_query(rs._h, p_v, n, hashes, p_rank, p_bit, memc, stream))
            pos = (v % np.uint64(BITS)).astype(np.int64)
            assert_same("rank_out n=%d hashes=%d" % (n, hashes), rank, csum[pos])
            assert_same("bit_out n=%d hashes=%d" % (n, hashes), bit, bits[pos])
    reg.check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_kmer_calls(direct, monkeypatch, byte, mem):
    """btlbf_hash_kmers and btlbf_contains_kmers with k-mers that have no defined value: valid 0, contains 0, hashes 0"""
    reg = poisoned_outputs(monkeypatch, byte)
    L, lib, o = direct.bf._lib.load(), direct.bf._lib, direct.oracle
    k, h, bits = 22, 3, 1 << 16
    rng = np.random.RandomState(9)
    alpha = list(b"ACGT" * 6 + b"UN")
    ins = bytes(rng.choice(alpha, k * 600).tolist())
    ihv, iok = o.kmer_hashes(ins, k, h)
    mine = np.zeros(bits // 8, np.uint8)
    o.bf_insert(mine, bits, h, ihv[iok == 1])
    f = direct.bf.KmerBloomFilter(bits, h, k)
    f.upload(mine)
    undefined = 0
    for n in ROW_NS:
        q = bytes(rng.choice(alpha, k * (n - n // 2)).tolist()) + ins[: (n // 2) * k]
        hv, ok = o.kmer_hashes(q, k, h)
        keep, p_q, memc, stream, dev = raw_in(np.frombuffer(q, np.uint8), mem)
        rows, p_rows = reg.alloc((n, h), np.uint64, dev, "hash_kmers hashes n=%d" % n)
        valid, p_valid = reg.alloc(n, np.uint8, dev, "hash_kmers valid n=%d" % n)
        lib.check(L.btlbf_hash_kmers(k, h, p_q, n, p_rows, p_valid, memc, 0, stream))
        assert_same("hash_kmers valid n=%d" % n, valid, ok)
        assert_same("hash_kmers hashes n=%d" % n, rows, hv)
        assert not hv[ok == 0].any()
        out, p_out = reg.alloc(n, np.uint8, dev, "contains_kmers n=%d" % n)
        lib.check(L.btlbf_contains_kmers(f._h, p_q, n, p_out, memc, stream))
        assert_same("contains_kmers n=%d" % n, out, o.bf_contains(mine, bits, h, hv) * ok)
        undefined += int((ok == 0).sum())
    assert undefined > 10
    reg.check_guards()


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_count_per_seq(direct, monkeypatch, byte, mem):
    """both outputs, one entry per sequence (empty ones included), ragged and uniform"""
    poisoned_outputs(monkeypatch, byte)
    for name in ("ragged", "uniform_31", "uniform_150"):
        lay = next(x for x in direct.layouts if x.name == name)
        w = direct.win(lay, K, H)
        hit = spread(lay.n, w.idx, direct.oracle.bf_contains(direct.body, BITS, H, w.crows).astype(bool))
        hb, vb = full_bitmap(hit, lay.n), full_bitmap(w.clean, lay.n)
        st = lay.starts
        if mem == "device":
            hb, vb = to_dev(hb.view(np.int64)), to_dev(vb.view(np.int64))
            st = None if st is None else to_dev(st.astype(np.int64))
        hits, valid = direct.bf.engine.count_per_seq(hb, vb, lay.n, K, starts=st, read_len=lay.read_len)
        assert_same(name + " hits_out", hits, np.array([hit[lo:hi].sum() for lo, hi in lay.seqs], np.uint32))
        assert_same(name + " valid_out", valid, np.array([w.clean[lo:hi].sum() for lo, hi in lay.seqs], np.uint32))
    check_guards()


# ---------------------------------------------------------------------------------------------
# (e) miBF
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mibf_query_case(bf):
    """test_gpu_mibf.py::test_query_against_model with spaced seeds and uint16 ids: the filter, the query buffer of
    inserted and foreign reads, and the model's whole answer for max_miss = 1"""
    from test_gpu_mibf import dense_case, ragged, rows_of

    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, 2, C5_SEEDS, 4)
    m = bf.MIBloomFilter(f, 2)
    m.insertIDs(seq, ids, starts=starts)
    m.insertSaturation(seq, ids, starts=starts)
    foreign, fst = ragged(np.random.RandomState(3), 100, 40, 150, 0.02)
    q = np.concatenate([seq, foreign])
    qst = np.concatenate([starts, fst[1:] + starts[-1]]).astype(np.uint64)
    qrows, qvalid = rows_of(bf, q, 4, C5_SEEDS, starts=qst)
    values, match = mm.query(m.data(), ranks, qrows, qvalid, 1, True)
    return m, q, qst, values.astype(np.uint16), match, qvalid


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_mibf_query(mibf_query_case, monkeypatch, byte, mem):
    """values 0 everywhere but the hit positions of matching windows; match and valid in whole words; counts2"""
    m, q, qst, values, match, qvalid = mibf_query_case
    assert match.any() and (qvalid & ~match).any() and (values == 0).any() and (values != 0).any()
    poisoned_outputs(monkeypatch, byte)
    seq, st = (to_dev(q), to_dev(qst.astype(np.int64))) if mem == "device" else (q, qst)
    got_values, got_match, got_valid, cnt = m.query(seq, max_miss=1, starts=st, want_counts=True)
    assert_same("values", got_values, values)
    assert_bitmap("match_bits", got_match, match, len(q))
    assert_bitmap("valid_bits", got_valid, qvalid, len(q))
    assert_same("counts2", cnt, np.array([qvalid.sum(), match.sum()], np.uint64))
    check_guards()


def classify_expectation(bf, exp, max_results):
    """the model's results as the four whole output arrays: rows zero behind min(n_hits, max_results)"""
    n = len(exp)
    hits = np.zeros((n, max_results), bf.engine.HIT_DTYPE)
    n_hits, sat, ev = (np.zeros(n, np.uint32) for _ in range(3))
    for i, (res, s, e) in enumerate(exp):
        n_hits[i], sat[i], ev[i] = len(res), s, e
        for j, r in enumerate(res[:max_results]):
            hits[i, j] = tuple(r)
    return hits, n_hits, sat, ev


def check_classify(bf, got, exp, max_results, mostly_tails=True):
    want = classify_expectation(bf, exp, max_results)
    for name, g, w in zip(("hits", "n_hits", "sat_count", "eval_count"), got, want):
        assert_same(name, g, w)
    n_hits = want[1]
    print("n_hits:", np.bincount(n_hits).tolist(), "max_results", max_results)
    assert (n_hits < max_results).sum() * 2 > len(n_hits) or not mostly_tails, "most rows have a tail"
    assert (n_hits < max_results).any() and (n_hits > max_results).any(), "a row with a tail, a truncated row"
    assert (want[3] == 0).any() and ((want[2] > 0).any() or not mostly_tails)  # no frame at all; saturated frames
    check_guards()


P_CLASSIFY = (1.0, 2, 1, 1, 0)  # extra_count, extra_frame_limit, max_miss = 1, min_frames, best_hit_agree
MAX_RESULTS = 2


@pytest.fixture(scope="module")
def classify_case(bf):
    """test_gpu_mibf_classify.py's C5 case with uint16 ids whose genomes share their middle among four neighbours (reads
    from there have up to four results), its edge reads, and the model's answers (computed with zeroed outputs)"""
    from test_gpu_mibf_classify import Case

    case = Case(bf, "C5", 2, 40, share=4)
    g = case.reads
    reads = [g[0][:K - 1], np.full(60, ord("N"), np.uint8), np.zeros(0, np.uint8), g[1][:K]] + g
    return case, reads, case.model(reads, P_CLASSIFY)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_mibf_classify(bf, classify_case, monkeypatch, byte, mem):
    case, reads, exp = classify_case
    ec, lim, mx, mc, agree = P_CLASSIFY
    seq = np.concatenate(reads)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
    if mem == "device":
        seq, starts = to_dev(seq), to_dev(starts.astype(np.int64))
    poisoned_outputs(monkeypatch, byte)
    got = case.m.classify(seq, case.prob, case.minc, extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_frames=mc,
                          best_hit_agree=bool(agree), max_results=MAX_RESULTS, starts=starts)
    check_classify(bf, got, exp, MAX_RESULTS)


@pytest.fixture(scope="module")
def pair_case(bf):
    from test_gpu_mibf_classify_pairs import PairCase, edge_pairs, model

    case = PairCase(bf, "C5", 2)
    pairs = edge_pairs(case) + case.pairs
    return case, pairs, model(case, pairs, P_CLASSIFY)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", MEMS)
def test_mibf_classify_pairs(bf, pair_case, monkeypatch, byte, mem):
    case, pairs, exp = pair_case
    ec, lim, mx, mc, agree = P_CLASSIFY
    seq, starts = bf.interleave_mates([a for a, _ in pairs], [b for _, b in pairs])
    if mem == "device":
        seq, starts = to_dev(seq), to_dev(starts.astype(np.int64))
    poisoned_outputs(monkeypatch, byte)
    got = case.m.classifyPairs(seq, case.prob, case.minc, extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_frames=mc,
                               best_hit_agree=bool(agree), max_results=1, starts=starts)
    check_classify(bf, got, exp, 1, mostly_tails=False)  # (one record per row: only rows without a result have a tail)


@pytest.mark.parametrize("byte", POISONS)
def test_mibf_frame_probs_leaves_entry_0(bf, classify_case, monkeypatch, byte):
    """frame_probs[0] is documented as NOT written: it keeps the poison; entries 1.. are written"""
    case = classify_case[0]
    want, want_sat = case.m.calcFrameProbs(case.n_ids, 1)
    reg = poisoned_outputs(monkeypatch, byte)
    probs, p_probs = reg.alloc(case.n_ids, np.float64, None, "frame_probs")
    sat = C.c_double()
    bf._lib.check(bf._lib.load().btlbf_mibf_frame_probs(case.m._h, 1, p_probs, case.n_ids, C.byref(sat)))
    assert (host_bytes(probs[:1]) == byte).all()
    assert_same("frame_probs[1:]", probs[1:], want[1:])
    assert sat.value == want_sat and (want[1:] > 0).any()
    reg.check_guards()
