"""BTLBF_DEVICE calls on a non-blocking stream whose inputs are still in flight, and BTLBF_HOST calls on such a stream
(include/btlbf.h, "streams": a DEVICE call reads its inputs and writes its outputs in the order of `stream`).

Every other GPU test runs with torch's default stream current -- the legacy NULL stream, which waits for every blocking
stream -- and with inputs settled long before the call: a kernel or memset launched on stream 0 instead of `s`, a
blocking hipMemcpy that reads a caller's device array before the caller's stream has produced it, or a result finished
on a side stream and never joined back cannot be seen there.  Here each case (tests/stream_gate.py) issues ONE call
under `with torch.cuda.stream(s):` with stream=None, the production idiom, while every device input still holds a DECOY
-- a valid input of the same shape: other reads, another ascending `starts` with the same ends, other ids, other hash
rows, other tables -- and the real input arrives behind a delay queued on `s`.  The precondition, asserted in every
case: the gate has not opened when the call is issued.  Afterwards the test does not synchronise the device: it queues
clone() of every output and of every guard band on `s`, waits for `s` alone and compares the clones.  Outputs are dirty
and guarded (tests/poison.py, both POISONS); those the engine allocates inside the call are filled on `s` by the call
itself, those of the raw ctypes calls before the delay.  A call without a device output (the inserts) is judged by the
filter body, read after `s` has been waited for.  Each case first runs with settled inputs: the same check, and the host
time of the call.

Expected values are the suite's own: the CPU oracle, tests/mibf_model.py, mibf_classify_model.py, mibf_tally_model.py,
wide_counter_model.py, judge_model.py, update_order_model.py; for the forced partitioned and the AUTO split routes the
direct kernel on the NULL stream with settled inputs and a full synchronisation (tests/test_gpu_parity.py pins it to
the oracle).  Everything is integer-exact except the stated inequalities of the parallel incrementMin.

Measured on an MI355X (the STREAM_GATE lines this file prints): the gate's delay of 50 ms, torch.cuda._sleep calibrated
with HIP events, runs 49.8 .. 50.0 ms; a blocking copy on the NULL stream beside a delay on the gate's stream returns in
0.04 ms (stream_gate.pick_stream: the two do not share a hardware queue); no case needed its second attempt.  The
longest host time of a call with settled inputs is 56 ms (the serial incrementMin of 300 reads: one lane, and the call
waits for it); then 9.5 ms (the serial miBF saturation in batches), 5.5 ms (insertSeqs + store) and below 3 ms for
every other call, most of them below 0.3 ms.
Returned BEFORE the gate opened, that is, asynchronous: insertSeqs, containsSeqs and insertAndCheckSeqs (direct, and
the forced partitioned query), the hash-row forms, the counting filters' parallel updates and queries (8 and 32 bits,
the partitioned incrementAll on an uploaded body included), rank_query, count_per_seq, and_answers, synth_reads,
classify_tally, and the direct first use of a fresh filter followed by a partitioned query on a second stream.
Returned after it, because they wait for the stream: everything BTLBF_HOST; hash_seqs, sthash_seqs and hash_kmers; the
raw k-mer forms; the fresh (first-use) partitioned insert; the AUTO split queries (the sampler's answer comes back to
the host); the serial counting update; popcount_bits; every miBF call except classify_tally; and the judges.

Without the fix of mibf_prepare (a scratch build with that one hunk reverted, run on the MI355X: the decoys are valid
layouts, so nothing can be read out of range) every `batched` miBF case below fails -- insert_ids and the serial
saturation with other counts and ids, classify, classify_pairs and interleave_mates + classify_pairs with other rows
(235 .. 541 result bytes differ) --, 18 cases, and the `one_batch` ones pass: with a single batch the kernels use the
call's own device offsets, and the host's early copy only sizes the scratch.
"""
import ctypes as C

import numpy as np
import pytest

import judge_model as jm
import mibf_model as mm
import test_gpu_mibf as tm
import test_gpu_output_contract as oc
import update_order_model as uo
import wide_counter_model as wm
from mibf_tally_model import tally_model
from poison import POISONS, assert_bitmap, assert_same, full_bitmap, host_bytes
from stream_gate import calibrate, run_gated, to_device
from test_gpu_auto_query import _assert_path, bf, splice  # noqa: F401  (bf: fixture)
from test_gpu_mibf_classify import Case
from test_gpu_mibf_classify_pairs import PairCase, edge_pairs
from test_gpu_mibf_classify_pairs import model as pair_model
from test_gpu_mibf_classify_tally import results as tally_results
from test_gpu_output_contract import split_filter  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

K, H, BITS = 31, 4, 1 << 22             # the bit filter
CSIZE, CK, CH, THR = 1 << 20, 25, 3, 2  # the 8-bit counting filter
L = 150
C5 = oc.C5_SEEDS


@pytest.fixture(scope="module")
def delay(bf):  # noqa: F811
    d = calibrate()
    print("STREAM_GATE delay kind=%s measured_ms=%.2f null_stream_copy_beside_10ms_delay_ms=%.3f" % (d.kind, d.measured_ms, d.null_copy_ms))
    return d


def u8(b):
    return np.frombuffer(b, np.uint8)


def cur(t):
    """the hipStream_t of a raw call: torch's current stream on the tensor's device, as the engine passes it"""
    from btl_bloomfilter_amd import engine

    return engine._stream_ptr(None, t)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def other_starts(starts):
    """another valid layout of the same bytes: the same sequence lengths in reverse order"""
    s = np.asarray(starts).astype(np.int64)
    out = np.concatenate([[0], np.cumsum(np.diff(s)[::-1])]).astype(np.uint64)
    assert out[-1] == s[-1] and (out != s.astype(np.uint64)).any()
    return out


def bits_of(words, n):
    return np.unpackbits(host_bytes(words), bitorder="little")[:n].astype(bool)


# ---------------------------------------------------------------------------------------------
# 1. hash streams
# ---------------------------------------------------------------------------------------------
HASH_LENS = [0, 30, 31, 2047, 2049, 4100, 2048, 32, 150, 151, 77, 64, 65, 0, 31, 2046, 100, 29] + [150, 149] * 11


class HashCase:
    def __init__(self, oracle):
        rng = np.random.RandomState(71)
        self.lay = oc.Layout(rng, "late_ragged", HASH_LENS, "ragged")
        self.dec = oc.Layout(rng, "decoy_ragged", HASH_LENS[::-1], "ragged")
        assert len(HASH_LENS) == 40 and self.lay.n == self.dec.n and (self.lay.starts != self.dec.starts).any()
        self.win = oc.Windows(oracle, self.lay.buf, self.lay.seqs, K, H)
        self.swin = oc.Windows(oracle, self.lay.buf, self.lay.seqs, K, H, C5)


@pytest.fixture(scope="module")
def hashes(oracle):
    return HashCase(oracle)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("spaced", [False, True], ids=["hash_seqs", "sthash_seqs"])
def test_hash_streams(bf, delay, hashes, monkeypatch, byte, spaced):  # noqa: F811
    """ragged: the sequence bytes and the device `starts` are late"""
    lay, dec = hashes.lay, hashes.dec
    w = hashes.swin if spaced else hashes.win

    def setup(g):
        seq = g.late(None, u8(lay.buf), u8(dec.buf))
        st = g.late(None, lay.starts, dec.starts)
        if spaced:
            return lambda: bf.sthash_seqs(seq, C5, 1, K, starts=st)
        return lambda: bf.hash_seqs(seq, H, K, starts=st)

    def check(got, note):
        assert_same(note + ": hashes", got[0], w.rows)
        assert_bitmap(note + ": valid_bits", got[1], w.clean, lay.n)
        if spaced:
            assert_same(note + ": strand_bits", got[2], w.strand)

    run_gated("sthash_seqs" if spaced else "hash_seqs", delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
def test_hash_kmers(bf, delay, oracle, monkeypatch, byte):  # noqa: F811
    k, h, n = 22, 3, 1000
    rng = np.random.RandomState(9)
    alpha = list(b"ACGT" * 6 + b"UN")
    q, dq = bytes(rng.choice(alpha, k * n).tolist()), bytes(rng.choice(alpha, k * n).tolist())
    hv, ok = oracle.kmer_hashes(q, k, h)
    L_, lib = bf._lib.load(), bf._lib

    def setup(g):
        src = g.late(None, u8(q), u8(dq))
        rows, p_rows = g.alloc((n, h), np.uint64, "hash_kmers hashes")
        valid, p_valid = g.alloc(n, np.uint8, "hash_kmers valid")

        def call():
            lib.check(L_.btlbf_hash_kmers(k, h, ptr(src), n, p_rows, p_valid, lib.DEVICE, 0, cur(src)))
            return rows, valid
        return call

    def check(got, note):
        assert_same(note + ": valid", got[1], ok)
        assert_same(note + ": hashes", got[0], hv)

    assert (ok == 0).any() and (ok == 1).any()
    run_gated("hash_kmers", delay, setup, check, monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 2. bit filter, direct: 2^22 bits, 2000 reads of 150
# ---------------------------------------------------------------------------------------------
class BitCase:
    def __init__(self, bf, oracle):  # noqa: F811
        rng = np.random.RandomState(72)
        self.lay = oc.Layout(rng, "u150", [L] * 2000, "uniform")
        self.dec = oc.Layout(rng, "u150_decoy", [L] * 2000, "uniform")
        self.n = self.lay.n
        self.body = np.zeros(BITS // 8, np.uint8)  # half of the reads are in the filter the queries see
        for s in self.lay.inserted:
            oracle.bf_insert_seq(self.body, BITS, H, K, s)
        self.win = w = oc.Windows(oracle, self.lay.buf, self.lay.seqs, K, H)
        self.hit = oc.spread(self.n, w.idx, oracle.bf_contains(self.body, BITS, H, w.crows).astype(bool))
        self.after = self.body.copy()               # the body after every read has been inserted into it ...
        oracle.bf_insert(self.after, BITS, H, w.crows)
        self.alone = np.zeros(BITS // 8, np.uint8)  # ... and into an empty filter
        oracle.bf_insert(self.alone, BITS, H, w.crows)
        self.rows = np.ascontiguousarray(w.crows[:20000])  # the hash-row forms (the serial one runs on one lane)
        self.rows_decoy = self.rows ^ np.uint64(0x5555555555555555)
        self.flt = self.filter(bf)
        self.twin = bf.BloomFilter(BITS, H, K)      # the judges' settled twin
        self.twin.upload(self.alone)

    def filter(self, bf, body=None):  # noqa: F811
        f = bf.BloomFilter(BITS, H, K)
        f.upload(self.body if body is None else body)
        return f


@pytest.fixture(scope="module")
def bitcase(bf, oracle):  # noqa: F811
    c = BitCase(bf, oracle)
    assert c.hit.sum() > 50000 and (c.win.clean & ~c.hit).sum() > 50000
    return c


def test_insert_seqs(bf, delay, bitcase):  # noqa: F811
    """the first use of a fresh filter: its lazy clear is carried out on `s` as well"""
    c = bitcase

    def setup(g):
        f = bf.BloomFilter(BITS, H, K)
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))
        return (lambda: f.insertSeqs(seq, read_len=L)), f.download

    def check(got, note):
        assert_same(note + ": filter body", got[0], c.alone)

    run_gated("insertSeqs", delay, setup, check)


@pytest.mark.parametrize("byte", POISONS)
def test_contains_seqs(delay, bitcase, monkeypatch, byte):
    c = bitcase

    def setup(g):
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))
        return lambda: c.flt.containsSeqs(seq, read_len=L, want_valid=True, want_counts=True)

    run_gated("containsSeqs", delay, setup, lambda got, note: oc.check_query(note, got, c.n, c.win.clean, c.hit, True, True),
              monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
def test_insert_and_check_seqs(bf, delay, bitcase, monkeypatch, byte):  # noqa: F811
    c = bitcase
    monkeypatch.setattr(oc, "BITS", BITS)  # (insert_and_check_expectation reduces the rows modulo its module's size)
    hit, amb = oc.insert_and_check_expectation(c.body, c.win, c.n)
    assert amb.sum() * 20 < (c.win.clean & ~hit & ~amb).sum()

    def setup(g):
        f = c.filter(bf)
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))
        return (lambda: f.insertAndCheckSeqs(seq, read_len=L, want_valid=True, want_counts=True)), f.download

    def check(got, note):
        want = np.where(amb, bits_of(got[0], c.n), hit)
        oc.check_query(note, got[:3], c.n, c.win.clean, want, True, True)
        assert_same(note + ": filter body", got[3], c.after)

    run_gated("insertAndCheckSeqs", delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("form", ["insert", "contains", "insertAndCheck"])
def test_hash_row_forms(bf, delay, oracle, bitcase, monkeypatch, byte, form):  # noqa: F811
    c = bitcase
    mine = c.body.copy()
    if form == "contains":
        want = oracle.bf_contains(mine, BITS, H, c.rows)
    else:
        want = oracle.bf_insert_and_check(mine, BITS, H, c.rows)  # (serial order: the oracle's loop; `mine` is the body after)
    assert 0 < want.sum() < len(want)

    def setup(g):
        f = c.flt if form == "contains" else c.filter(bf)
        rows = g.late(None, c.rows, c.rows_decoy)
        if form == "insert":
            return (lambda: f.insert(rows)), f.download
        if form == "contains":
            return lambda: f.contains(rows)
        return (lambda: f.insertAndCheck(rows, serial=True)), f.download

    def check(got, note):
        if form != "insert":
            assert_same(note + ": out", got[0], want)
        if form != "contains":
            assert_same(note + ": filter body", got[-1], mine)

    run_gated(form + "_hashes", delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("form", ["insertKmers", "containsKmers"])
def test_kmer_forms(bf, delay, oracle, monkeypatch, byte, form):  # noqa: F811
    k, h, n = 22, 3, 2000
    rng = np.random.RandomState(10)
    alpha = list(b"ACGT" * 6 + b"UN")
    ins = bytes(rng.choice(alpha, k * n).tolist())
    q = bytes(rng.choice(alpha, k * (n // 2)).tolist()) + ins[: (n - n // 2) * k]
    dq = bytes(rng.choice(alpha, k * n).tolist())
    ihv, iok = oracle.kmer_hashes(ins, k, h)
    qhv, qok = oracle.kmer_hashes(q, k, h)
    mine = np.zeros(BITS // 8, np.uint8)
    oracle.bf_insert(mine, BITS, h, ihv[iok == 1])
    want = oracle.bf_contains(mine, BITS, h, qhv) * qok
    after = mine.copy()
    oracle.bf_insert(after, BITS, h, qhv[qok == 1])
    assert 0 < want.sum() < n and (qok == 0).any() and (after != mine).any()

    def setup(g):
        f = bf.KmerBloomFilter(BITS, h, k)
        f.upload(mine)
        src = g.late(None, u8(q), u8(dq))
        if form == "insertKmers":
            return (lambda: f.insertKmers(src)), f.download
        return lambda: f.containsKmers(src)

    def check(got, note):
        assert_same(note, got[0], after if form == "insertKmers" else want)

    run_gated(form, delay, setup, check, monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 3. forced partitioned insert and query (2^22 bits, 20 000 reads), the AUTO split query
# ---------------------------------------------------------------------------------------------
N3 = 20000


class PartCase:
    """the reads, a query buffer with every 10th read foreign and one N, and the direct kernel's answers on the NULL
    stream with settled inputs and a full synchronisation"""

    def __init__(self, bf):  # noqa: F811
        import torch

        self.reads = bf.synth_reads_device(42, 0, N3, L)
        self.other = bf.synth_reads_device(44, 0, N3, L)
        self.q = splice(bf, self.reads.clone(), N3, L, np.arange(0, N3, 10))
        self.q[12345] = ord("N")
        self.starts = (np.arange(N3 + 1) * L).astype(np.uint64)
        dec = self.starts.astype(np.int64)
        dec[1:-1] -= (np.arange(1, N3) % 2) * 7  # another ascending layout of the same bytes
        self.starts_decoy = dec.astype(np.uint64)
        d = bf.BloomFilter(BITS, H, K)
        d.setInsertMode("direct")
        d.setQueryMode("direct")
        d.insertSeqs(self.reads, read_len=L)
        torch.cuda.synchronize()
        self.body = d.download()
        self.answer = [oc._np(x) for x in d.containsSeqs(self.q, read_len=L, want_valid=True, want_counts=True)]
        torch.cuda.synchronize()
        cnt = self.answer[2].tolist()
        assert 0 < cnt[1] < cnt[0] == N3 * (L - K + 1) - K


@pytest.fixture(scope="module")
def part(bf):  # noqa: F811
    return PartCase(bf)


@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_forced_partitioned_insert(bf, delay, part, layout):  # noqa: F811
    def setup(g):
        f = bf.BloomFilter(BITS, H, K)
        f.setInsertMode("partitioned")
        f.setProfiling(True)
        seq = g.late(None, part.reads, part.other)
        kw = dict(read_len=L) if layout == "uniform" else dict(starts=g.late(None, part.starts, part.starts_decoy))
        return (lambda: f.insertSeqs(seq, **kw)), (lambda: (f.download(), f.getProfile()))

    def check(got, note):
        body, prof = got
        assert_same(note + ": filter body", body, part.body)
        assert "insert_apply" in prof and "insert_direct" not in prof, (note, prof)

    run_gated("insertSeqs partitioned " + layout, delay, setup, check)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("layout", ["uniform", "ragged"])
def test_forced_partitioned_query(bf, delay, part, monkeypatch, byte, layout):  # noqa: F811
    f = bf.BloomFilter(BITS, H, K)
    f.upload(part.body)
    f.setQueryMode("partitioned")
    f.setProfiling(True)
    n = part.q.numel()

    def setup(g):
        f.getProfile()
        seq = g.late(None, part.q, part.reads)
        kw = dict(read_len=L) if layout == "uniform" else dict(starts=g.late(None, part.starts, part.starts_decoy))
        return (lambda: f.containsSeqs(seq, want_valid=True, want_counts=True, **kw)), f.getProfile

    def check(got, note):
        assert_bitmap(note + ": hit_bits", got[0], bits_of(part.answer[0], n), n)
        assert_bitmap(note + ": valid_bits", got[1], bits_of(part.answer[1], n), n)
        assert_same(note + ": counts", got[2], part.answer[2])
        oc.partitioned_ran(1)(got[3], note)

    run_gated("containsSeqs partitioned " + layout, delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("route", ["split_cold", "split_warm"])
def test_auto_split_query(bf, delay, split_filter, monkeypatch, byte, route):  # noqa: F811
    """the shape at which tests/test_gpu_output_contract.py has the sampler choose the two split routes; a decoy of
    inserted reads alone would send the whole buffer to the partitioned query"""
    import torch

    flt, reads, n, L3 = split_filter
    foreign = np.arange(0, n, 10) if route == "split_cold" else np.arange(n // 3) * 3 + 1
    q = splice(bf, reads[: n * L3].clone(), n, L3, foreign)
    nb = q.numel()
    flt.setQueryMode("direct")
    want = [oc._np(x) for x in flt.containsSeqs(q, read_len=L3, want_valid=True, want_counts=True)]
    torch.cuda.synchronize()
    flt.setQueryMode("auto")
    flt.setProfiling(True)

    def setup(g):
        flt.getProfile()
        seq = g.late(None, q, reads[: n * L3])
        return (lambda: flt.containsSeqs(seq, read_len=L3, want_valid=True, want_counts=True)), flt.getProfile

    def check(got, note):
        assert_bitmap(note + ": hit_bits", got[0], bits_of(want[0], nb), nb)
        assert_bitmap(note + ": valid_bits", got[1], bits_of(want[1], nb), nb)
        assert_same(note + ": counts", got[2], want[2])
        _assert_path(got[3], route, 1, False)

    try:
        run_gated("containsSeqs auto " + route, delay, setup, check, monkeypatch, byte)
    finally:
        flt.setProfiling(False)


# ---------------------------------------------------------------------------------------------
# 4. counting filters
# ---------------------------------------------------------------------------------------------
class CountCase:
    """300 reads of 150 into 2^20 prefilled 8-bit counters (k = 25, h = 3, threshold 2)"""

    def __init__(self, bf, oracle):  # noqa: F811
        rng = np.random.RandomState(73)
        self.lay = oc.Layout(rng, "c150", [L] * 300, "uniform")
        self.dec = oc.Layout(rng, "c150_decoy", [L] * 300, "uniform")
        self.n = self.lay.n
        self.win = w = oc.Windows(oracle, self.lay.buf, self.lay.seqs, CK, CH)
        self.before = uo.prefilled_counters(5, CSIZE)
        self.pos = uo.positions(w.crows, CSIZE)
        self.all = self.before.copy()
        oracle.cbf_increment_all(self.all, CH, w.crows)
        self.min_serial = self.before.copy()
        oracle.cbf_increment_min(self.min_serial, CH, w.crows)
        mn, ct = oracle.cbf_query(self.before, CH, THR, w.crows)
        self.want_min = oc.spread(self.n, w.idx, mn, np.uint8)
        self.hit = oc.spread(self.n, w.idx, ct.astype(bool))
        assert {0, 1, 2} <= set(mn.tolist()) and 0 < self.hit.sum() < w.clean.sum()
        self.flt = self.filter(bf)

    def filter(self, bf):  # noqa: F811
        f = bf.CountingBloomFilter(CSIZE, CH, CK, THR)
        f.upload(self.before)
        return f


@pytest.fixture(scope="module")
def countcase(bf, oracle):  # noqa: F811
    return CountCase(bf, oracle)


@pytest.mark.parametrize("op", ["all_direct", "all_partitioned", "min_serial", "min_parallel"])
def test_counting_updates(bf, delay, countcase, op):  # noqa: F811
    c = countcase

    def setup(g):
        f = c.filter(bf)
        f.setInsertMode("partitioned" if op == "all_partitioned" else "direct")
        f.setProfiling(True)
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))
        kw = dict(increment_all=op.startswith("all"), serial=op == "min_serial")
        return (lambda: f.insertSeqs(seq, read_len=L, **kw)), (lambda: (f.download(), f.getProfile()))

    def check(got, note):
        body, prof = got
        try:
            if op.startswith("all"):
                uo.check_increment_all(body, c.all)
            elif op == "min_serial":
                assert_same(note + ": counters", body, c.min_serial)
            else:  # the atomic contract (M1-M4), not equality
                uo.check_increment_min(c.before, body, c.all, c.pos)
        except uo.ContractViolation as e:
            pytest.fail("%s: %s" % (note, e))
        assert ("insert_apply" in prof) == (op == "all_partitioned"), (note, prof)

    run_gated("counting insertSeqs " + op, delay, setup, check)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("call", ["minCountSeqs", "containsSeqs"])
def test_counting_queries(delay, countcase, monkeypatch, byte, call):
    c = countcase

    def setup(g):
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))
        if call == "minCountSeqs":
            return lambda: c.flt.minCountSeqs(seq, read_len=L)
        return lambda: c.flt.containsSeqs(seq, read_len=L, want_valid=True, want_counts=True)

    def check(got, note):
        if call == "minCountSeqs":
            assert_same(note + ": min_out", got[0], c.want_min)
            assert_bitmap(note + ": valid_bits", got[1], c.win.clean, c.n)
        else:
            oc.check_query(note, got, c.n, c.win.clean, c.hit, True, True)

    run_gated("counting " + call, delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("call", ["incrementAll", "minCountSeqs"])
def test_wide_counters_32(bf, delay, oracle, monkeypatch, byte, call):  # noqa: F811
    """the model's seeded 1000-byte case, ragged, bytes and device `starts` late"""
    bits = 32
    nbytes, h, k, thr, reads, before = wm.make_case("c1000", bits)
    buf, dbuf = b"".join(reads), b"".join(reads[::-1])
    starts = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    wpos, wrows = uo.clean_windows(oracle, buf, k, h, starts=starts)
    b = np.frombuffer(before, wm.DTYPES[bits]).astype(np.uint64)
    model = wm.WideCBF(bits, nbytes, h, k, thr, before)
    want_all = wm.increment_all_exact(b, uo.positions(wrows, model.size), wm.max_of(bits))
    want_min = np.zeros(len(buf), np.uint64)
    want_min[wpos] = [model.min_count(r) for r in wrows]
    clean = np.zeros(len(buf), bool)
    clean[wpos] = True
    assert (want_min > 255).any() and (want_all != b).any()

    def setup(g):
        f = bf.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
        f.upload(u8(before))
        seq = g.late(None, u8(buf), u8(dbuf))
        st = g.late(None, starts, other_starts(starts))
        if call == "incrementAll":
            return (lambda: f.insertSeqs(seq, starts=st, increment_all=True)), f.counters
        return lambda: f.minCountSeqs(seq, starts=st)

    def check(got, note):
        if call == "incrementAll":
            wm.check_increment_all(got[0], want_all)
        else:
            assert_same(note + ": min_out", got[0], want_min.astype(wm.DTYPES[bits]))
            assert_bitmap(note + ": valid_bits", got[1], clean, len(buf))

    run_gated("32-bit " + call, delay, setup, check, monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 5. a fresh filter: first use on s1, then a query on s2 behind s2.wait_stream(s1)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("first,second", [("partitioned", "direct"), ("direct", "partitioned")])
def test_fresh_filter_first_use_then_another_stream(bf, delay, part, monkeypatch, byte, first, second):  # noqa: F811
    """creation is a lazy clear; whichever stream makes the first use zeroes the array (or, partitioned, builds every
    segment from zero), and a second stream, ordered behind the first by an event and by no host synchronisation, sees
    the zeroed array and the insert.  The test's own s2.wait_stream(s1) already orders s2 behind the zeroing, so the wait
    of materialize_clear for zero_ev is redundant here and its absence would not show: what the case checks is that the
    zero_ev / clear_ev paths, taken from a stream other than the one that zeroed, do no harm and lose nothing."""
    import torch

    nb = N3 * L
    valid = (np.arange(nb) % L) <= L - K  # synthetic reads hold no unclean byte: every window of every read

    def setup(g):
        f = bf.BloomFilter(BITS, H, K)
        f.setInsertMode(first)
        f.setQueryMode(second)
        f.setProfiling(True)
        seq = g.late(None, part.reads, part.other)
        s2 = torch.cuda.Stream()
        for _ in range(32):  # torch hands side streams out of a pool, round-robin: the gate's own may come up again
            if s2.cuda_stream != g.s.cuda_stream:
                break
            s2 = torch.cuda.Stream()
        assert s2.cuda_stream != g.s.cuda_stream, "the second stream is the gate's stream: one stream, not two"

        def call():
            f.insertSeqs(seq, read_len=L)
            s2.wait_stream(g.s)
            with torch.cuda.stream(s2):
                outs = f.containsSeqs(seq, read_len=L, want_valid=True, want_counts=True)
            g.s.wait_stream(s2)  # (the consumer of stream_gate clones on g.s)
            return outs
        return call, f.getProfile

    def check(got, note):
        assert_bitmap(note + ": valid_bits", got[1], valid, nb)
        assert_bitmap(note + ": hit_bits", got[0], valid, nb)  # every clean window hits
        assert_same(note + ": counts", got[2], np.array([valid.sum()] * 2, np.uint64))
        prof = got[3]
        assert ("insert_apply" in prof) == (first == "partitioned") and ("query_hash" in prof) == (second == "partitioned"), (note, prof)

    run_gated("fresh filter %s insert, %s query" % (first, second), delay, setup, check, monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 6. the judges after asynchronous work
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("judge", ["download", "popcount", "digest", "compare", "store", "rank_create", "mibf_create",
                                   "microbench"])
def test_judges_wait_for_user_streams(bf, delay, bitcase, tmp_path, judge):  # noqa: F811
    """a gated insertSeqs on `s`, then -- with no synchronisation by the test -- a host-visible call that claims to wait
    for user streams: it sees the oracle's body, and the gate has opened when it returns.  btlbf_microbench (kind 0: loads
    from the array on the NULL stream, which change nothing) has no result to compare: it must have waited, and the body
    read after it is the oracle's"""
    from btl_bloomfilter_amd.engine import body_digest

    c = bitcase
    pop = jm.dense_popcount(c.alone, 0)
    c.twin.storeFilter(tmp_path / "twin.bf")

    def setup(g):
        f = bf.BloomFilter(BITS, H, K)
        seq = g.late(None, u8(c.lay.buf), u8(c.dec.buf))

        def call():
            f.insertSeqs(seq, read_len=L)
            if judge == "download":
                r = f.download()
            elif judge == "popcount":
                r = f.getPop()
            elif judge == "digest":
                r = f.digest()
            elif judge == "compare":
                r = f.compare(c.twin)
            elif judge == "store":
                f.storeFilter(tmp_path / "f.bf")
                r = (tmp_path / "f.bf").read_bytes()
            elif judge == "rank_create":
                rs = bf.RankSupport(f)
                r = (rs.ones(), rs.interleaved())
            elif judge == "microbench":
                done, seconds = f.microbench(0, 1 << 22)
                assert not g.in_flight(), "btlbf_microbench returned while the stream of the insert had not reached the insert"
                assert done >= 1 << 22 and seconds > 0
                r = f.download()
            else:
                r = bf.MIBloomFilter(f, 2).getPop()
            assert not g.in_flight(), "%s returned while the stream of the insert had not reached the insert" % judge
            return [r]
        return call

    def check(got, note):
        r = got[0]
        if judge in ("download", "microbench"):
            assert_same(note, r, c.alone)
        elif judge == "popcount" or judge == "mibf_create":
            assert r == pop, note
        elif judge == "digest":
            assert r == body_digest(c.alone), note
        elif judge == "compare":
            assert r == (0, 0, 0), note
        elif judge == "store":
            assert r == (tmp_path / "twin.bf").read_bytes() and r.endswith(c.alone.tobytes()), note
        else:
            words = np.zeros((BITS // 512, 8), np.uint64)
            words[:] = c.alone.view("<u8").reshape(-1, 8)
            before = np.concatenate([[0], np.cumsum([jm.dense_popcount(blk, 0) for blk in c.alone.reshape(-1, 64)])])
            assert r[0] == pop == before[-1], note
            assert (r[1][:, 0] == before[:-1].astype(np.uint64)).all() and (r[1][:, 1:] == words).all(), note

    run_gated("insertSeqs then " + judge, delay, setup, check)


# ---------------------------------------------------------------------------------------------
# 7. rank and helpers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("values_are_hashes", [0, 1])
def test_rank_query(bf, delay, bitcase, monkeypatch, byte, values_are_hashes):  # noqa: F811
    c = bitcase
    L_, lib = bf._lib.load(), bf._lib
    rs = bf.RankSupport(c.flt)
    bits = np.unpackbits(c.body, bitorder="little")
    csum = np.zeros(BITS + 1, np.uint64)  # csum[p] = set bits before p
    csum[1:] = np.cumsum(bits, dtype=np.uint64)
    rng = np.random.RandomState(5)
    n = 1000
    hi = 2**63 if values_are_hashes else BITS
    v, dv = rng.randint(0, hi, n).astype(np.uint64), rng.randint(0, hi, n).astype(np.uint64)
    pos = (v % np.uint64(BITS)).astype(np.int64)

    def setup(g):
        src = g.late(None, v, dv)
        rank, p_rank = g.alloc(n, np.uint64, "rank_out")
        bit, p_bit = g.alloc(n, np.uint8, "bit_out")

        def call():
            lib.check(L_.btlbf_rank_query(rs._h, ptr(src), n, values_are_hashes, p_rank, p_bit, lib.DEVICE, cur(src)))
            return rank, bit
        return call

    def check(got, note):
        assert_same(note + ": rank_out", got[0], csum[pos])
        assert_same(note + ": bit_out", got[1], bits[pos])

    run_gated("rank_query hashes=%d" % values_are_hashes, delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
def test_count_per_seq(bf, delay, hashes, monkeypatch, byte):  # noqa: F811
    """both bitmaps and the device `starts` are late"""
    lay, dec, w = hashes.lay, hashes.dec, hashes.win
    hit = w.clean & (np.arange(lay.n) % 3 == 0)
    hb, vb = full_bitmap(hit, lay.n), full_bitmap(w.clean, lay.n)
    dhb, dvb = full_bitmap(w.clean & (np.arange(lay.n) % 3 == 1), lay.n), full_bitmap(np.arange(lay.n) % 2 == 0, lay.n)

    def setup(g):
        h, v, st = g.late(None, hb, dhb), g.late(None, vb, dvb), g.late(None, lay.starts, dec.starts)
        return lambda: bf.engine.count_per_seq(h, v, lay.n, K, starts=st)

    def check(got, note):
        assert_same(note + ": hits_out", got[0], np.array([hit[lo:hi].sum() for lo, hi in lay.seqs], np.uint32))
        assert_same(note + ": valid_out", got[1], np.array([w.clean[lo:hi].sum() for lo, hi in lay.seqs], np.uint32))

    run_gated("count_per_seq", delay, setup, check, monkeypatch, byte)


def test_popcount_bits(bf, delay):  # noqa: F811
    """a raw device buffer that is late; the count comes back to the host, so the call waits for `s`"""
    L_, lib = bf._lib.load(), bf._lib
    rng = np.random.RandomState(6)
    x, dx = rng.randint(0, 256, 1 << 20).astype(np.uint8), rng.randint(0, 256, 1 << 20).astype(np.uint8)

    def setup(g):
        src = g.late(None, x, dx)

        def call():
            out = C.c_uint64(0xA5A5A5A5A5A5A5A5)
            lib.check(L_.btlbf_popcount_bits(ptr(src), x.size, C.byref(out), 0, cur(src)))
            assert not g.in_flight()
            return [out.value]
        return call

    want = jm.dense_popcount(x, 0)
    assert want != jm.dense_popcount(dx, 0)
    run_gated("popcount_bits", delay, setup, lambda got, note: got[0] == want or pytest.fail("%s: %d, expected %d" % (note, got[0], want)))


@pytest.mark.parametrize("byte", POISONS)
def test_and_answers(bf, delay, monkeypatch, byte):  # noqa: F811
    """tags, answers and the bitmap the call updates are late: a 0 answer clears the bit of window tag / h"""
    L_, lib = bf._lib.load(), bf._lib
    rng = np.random.RandomState(8)
    n_win, h, n = 5000, 4, 15000
    tags, dtags = (rng.permutation(n_win * h)[:n].astype(np.uint64) for _ in range(2))
    ans, dans = (rng.randint(0, 2, n).astype(np.uint8) for _ in range(2))
    start = rng.rand(n_win) < 0.8
    want = start.copy()
    want[(tags[ans == 0] // np.uint64(h)).astype(np.int64)] = False
    assert 0 < want.sum() < start.sum()

    def setup(g):
        t, a = g.late(None, tags, dtags), g.late(None, ans, dans)
        out, _ = g.alloc((n_win + 63) // 64, np.uint64, "hit_bits")
        g.late(out, full_bitmap(start, n_win), full_bitmap(np.ones(n_win, bool), n_win))

        def call():
            lib.check(L_.btlbf_and_answers(ptr(t), ptr(a), n, h, ptr(out), 0, cur(t)))
            return [out]
        return call

    run_gated("and_answers", delay, setup, lambda got, note: assert_bitmap(note + ": hit_bits", got[0], want, n_win), monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
def test_synth_reads(bf, delay, oracle, monkeypatch, byte):  # noqa: F811
    """no input at all: the output, filled with poison on `s`, must be written on `s` behind the delay"""
    L_, lib = bf._lib.load(), bf._lib
    n = 1000
    want = oracle.synth_reads(42, 5, n, L)

    def setup(g):
        out, p_out = g.alloc(n * L, np.uint8, "synth_reads")

        def call():
            lib.check(L_.btlbf_synth_reads(p_out, 42, 5, n, L, 0, cur(out)))
            return [out]
        return call

    run_gated("synth_reads", delay, setup, lambda got, note: assert_same(note, got[0], want), monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 8. miBF: ragged layouts whose device `starts`, ids and tables are late
# ---------------------------------------------------------------------------------------------
MBITS = 1 << 18
P_CLASSIFY = oc.P_CLASSIFY
MAX_RESULTS = oc.MAX_RESULTS


class MibfCase:
    """60 ragged sequences over 2^18 bits with spaced seeds, the model's arrays after each stage, a query buffer of the
    inserted and of foreign sequences, and decoys: other bases, the lengths in reverse order, other ids"""

    def __init__(self, bf, id_bytes):  # noqa: F811
        self.id_bytes = id_bytes
        rng = np.random.RandomState(17 + id_bytes)
        self.seq, self.starts = tm.ragged(rng, 60, 60, 160, 0.005)
        self.ids = rng.randint(1, 40, 60)
        self.seq_decoy = tm.ragged(rng, 1, len(self.seq), len(self.seq) + 1, 0.005)[0]
        self.starts_decoy = other_starts(self.starts)
        self.ids_decoy = (self.ids + 7) % 39 + 1
        self.f = tm.stage1(bf, MBITS, 4, C5, self.seq, starts=self.starts)
        self.ranks = mm.Ranks(self.f.download(), MBITS)
        self.rows, self.valid = tm.rows_of(bf, self.seq, 4, C5, starts=self.starts)
        self.wseq = mm.window_seqs(len(self.seq), self.starts)
        pop = self.ranks.pop
        self.data1, self.counts1 = np.zeros(pop, np.int64), np.zeros(pop, np.int64)
        mm.insert_ids(self.data1, self.counts1, self.ranks, self.rows, self.valid, self.wseq, self.ids, id_bytes)
        self.sat = {}
        for serial in (True, False):
            d, c = self.data1.copy(), self.counts1.copy()
            fn = mm.saturate_serial if serial else mm.saturate_parallel
            self.sat[serial] = (fn(d, c, self.ranks, self.rows, self.valid, self.wseq, self.ids, id_bytes), d, c)
        # the query: on the filter after insertIDs and the parallel saturation
        self.m = self.inserted(bf)
        self.m.insertSaturation(self.seq, self.ids, starts=self.starts)
        foreign, fst = tm.ragged(rng, 20, 40, 150, 0.02)
        self.q = np.concatenate([self.seq, foreign])
        self.qst = np.concatenate([self.starts, fst[1:] + self.starts[-1]]).astype(np.uint64)
        self.q_decoy = tm.ragged(rng, 1, len(self.q), len(self.q) + 1, 0.02)[0]
        qrows, self.qvalid = tm.rows_of(bf, self.q, 4, C5, starts=self.qst)
        self.values, self.match = mm.query(self.m.data(), self.ranks, qrows, self.qvalid, 1, True)

    def inserted(self, bf):  # noqa: F811
        m = bf.MIBloomFilter(self.f, self.id_bytes)
        m.insertIDs(self.seq, self.ids, starts=self.starts)
        return m


@pytest.fixture(scope="module")
def mibfs(bf):  # noqa: F811
    return {b: MibfCase(bf, b) for b in (2, 4)}


def late_ragged(g, c):
    return (g.late(None, c.seq, c.seq_decoy), g.late(None, c.starts, c.starts_decoy),
            g.late(None, c.ids.astype(np.int32), c.ids_decoy.astype(np.int32)))


# A miBF call cuts its batches on the HOST's copy of `starts`.  With the default scratch budget these inputs are one batch,
# which runs on the call's own device offsets; under a small budget the batches' offsets are staged from the host's copy,
# and a copy taken before the stream had produced `starts` changes ids, counts and rows.  Both are run.
BUDGETS = {"one_batch": 0, "batched": 1}


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_mibf_insert_ids(bf, delay, mibfs, id_bytes, budget):  # noqa: F811
    c = mibfs[id_bytes]

    def setup(g):
        m = bf.MIBloomFilter(c.f, id_bytes)
        m.setScratchBudget(BUDGETS[budget] << 16)  # 2^16 bytes: about 500 bytes of sequence, a few sequences, per batch
        seq, st, ids = late_ragged(g, c)
        return (lambda: m.insertIDs(seq, ids, starts=st)), (lambda: (m.data(), m.counts()))

    def check(got, note):
        assert (got[1].astype(np.int64) == c.counts1).all(), note + ": counts"
        assert (got[0].astype(np.int64) == c.data1).all(), note + ": data"

    run_gated("mibf insert_ids_seqs %s u%d" % (budget, 8 * id_bytes), delay, setup, check)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("order", ["serial", "serial_batched", "parallel"])
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_mibf_saturate(bf, delay, mibfs, monkeypatch, byte, id_bytes, order):  # noqa: F811
    """serial_batched: 2^14 bytes of scratch, 496 bytes of sequence per batch (tests/test_gpu_mibf.py)"""
    c = mibfs[id_bytes]
    serial = order != "parallel"
    exp, data, counts = c.sat[serial]

    def setup(g):
        m = c.inserted(bf)
        m.setScratchBudget(1 << 14 if order == "serial_batched" else 0)
        seq, st, ids = late_ragged(g, c)
        return (lambda: [m.insertSaturation(seq, ids, starts=st, serial=serial)]), (lambda: (m.data(), m.counts()))

    def check(got, note):
        assert [got[0][x] for x in ("clean", "found", "mutated", "saturated")] == exp, note
        assert (got[2].astype(np.int64) == counts).all(), note + ": counts"
        assert (got[1].astype(np.int64) == data).all(), note + ": data"

    assert exp[0] > 0 and exp[1] > 0
    run_gated("mibf saturate_seqs %s u%d" % (order, 8 * id_bytes), delay, setup, check, monkeypatch, byte)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_mibf_query(delay, mibfs, monkeypatch, byte, id_bytes):
    c = mibfs[id_bytes]
    assert c.match.any() and (c.qvalid & ~c.match).any()

    def setup(g):
        seq, st = g.late(None, c.q, c.q_decoy), g.late(None, c.qst, other_starts(c.qst))
        return lambda: c.m.query(seq, max_miss=1, starts=st, want_counts=True)

    def check(got, note):
        assert_same(note + ": values", got[0], c.values.astype(c.m.dtype))
        assert_bitmap(note + ": match_bits", got[1], c.match, len(c.q))
        assert_bitmap(note + ": valid_bits", got[2], c.qvalid, len(c.q))
        assert_same(note + ": counts2", got[3], np.array([c.qvalid.sum(), c.match.sum()], np.uint64))

    run_gated("mibf query_seqs u%d" % (8 * id_bytes), delay, setup, check, monkeypatch, byte)


def late_tables(g, case):
    """perFrameProb and minCount on the device, late; the decoys are other probabilities and other minimum counts"""
    prob, minc = np.asarray(case.prob, np.float64), np.asarray(case.minc, np.int32)
    return g.late(None, prob, prob[::-1].copy()), g.late(None, minc, minc[::-1] + 1)


def classify_kw():
    ec, lim, mx, mc, agree = P_CLASSIFY
    return dict(extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_frames=mc, best_hit_agree=bool(agree))


def check_rows(bf, got, exp, max_results, note):  # noqa: F811
    want = oc.classify_expectation(bf, exp, max_results)
    for name, g_, w in zip(("hits", "n_hits", "sat_count", "eval_count"), got, want):
        assert_same("%s: %s" % (note, name), g_, w)


@pytest.fixture(scope="module")
def classify_cases(bf):  # noqa: F811
    """tests/test_gpu_mibf_classify.py's C5 case (2^18 bits, 40 ids whose genomes share their middle among four), its
    edge reads and 64 reads, for both id widths, with the model's answers"""
    out = {}
    for b in (2, 4):
        case = Case(bf, "C5", b, 40, share=4)
        g = case.reads
        reads = [g[0][:K - 1], np.full(60, ord("N"), np.uint8), np.zeros(0, np.uint8), g[1][:K]] + g
        out[b] = (case, reads, case.model(reads, P_CLASSIFY))
    return out


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_mibf_classify(bf, delay, classify_cases, monkeypatch, byte, id_bytes, budget):  # noqa: F811
    """batched: 4096 bytes of scratch, a few reads per batch (tests/test_gpu_mibf_classify.py)"""
    case, reads, exp = classify_cases[id_bytes]
    seq = np.concatenate(reads)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
    assert any(len(r[0]) > MAX_RESULTS for r in exp) and any(len(r[0]) == 0 for r in exp)

    def setup(g):
        s, st = g.late(None, seq, np.roll(seq, 37)), g.late(None, starts, other_starts(starts))
        prob, minc = late_tables(g, case)
        return lambda: case.m.classify(s, prob, minc, max_results=MAX_RESULTS, starts=st, **classify_kw())

    case.m.setScratchBudget(BUDGETS[budget] * 4096)
    try:
        run_gated("mibf classify_seqs %s u%d" % (budget, 8 * id_bytes), delay, setup,
                  lambda got, note: check_rows(bf, got, exp, MAX_RESULTS, note), monkeypatch, byte)
    finally:
        case.m.setScratchBudget(0)


@pytest.fixture(scope="module")
def pair_cases(bf):  # noqa: F811
    out = {}
    for b in (2, 4):
        case = PairCase(bf, "C5", b)
        pairs = edge_pairs(case) + case.pairs
        out[b] = (case, pairs, pair_model(case, pairs, P_CLASSIFY))
    return out


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_mibf_classify_pairs(bf, delay, pair_cases, monkeypatch, byte, id_bytes, budget):  # noqa: F811
    """the decoy `starts` is a different valid pairing of the same bytes: stale offsets change rows.  batched: 8192 bytes
    of scratch (the largest pair, two mates of 200 bases, costs 4128), one to three pairs per batch"""
    case, pairs, exp = pair_cases[id_bytes]
    seq, starts = bf.interleave_mates([a for a, _ in pairs], [b for _, b in pairs])
    assert any(len(r[0]) > 1 for r in exp) and any(len(r[0]) == 0 for r in exp)

    def setup(g):
        s, st = g.late(None, seq, seq.copy()), g.late(None, starts, other_starts(starts))
        prob, minc = late_tables(g, case)
        return lambda: case.m.classifyPairs(s, prob, minc, max_results=1, starts=st, **classify_kw())

    case.m.setScratchBudget(BUDGETS[budget] * 8192)
    try:
        run_gated("mibf classify_pairs %s u%d" % (budget, 8 * id_bytes), delay, setup,
                  lambda got, note: check_rows(bf, got, exp, 1, note), monkeypatch, byte)
    finally:
        case.m.setScratchBudget(0)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_interleave_mates_then_classify_pairs(bf, delay, pair_cases, monkeypatch, byte, id_bytes, budget):  # noqa: F811
    """the header's own composition on one stream with nothing in between: btlbf_interleave_mates (device) only queues
    its kernel, so the offsets classify_pairs plans its batches from do not exist yet when it is called.  The buffers
    between the two calls hold a valid decoy pairing until then."""
    from test_gpu_interleave_mates import ragged

    case, pairs, exp = pair_cases[id_bytes]
    L_, lib = bf._lib.load(), bf._lib
    r1, r2 = [a for a, _ in pairs], [b for _, b in pairs]
    (s1, st1), (s2, st2) = ragged(r1), ragged(r2)
    (d1, dst1), (d2, dst2) = ragged(r1[::-1]), ragged(r2[::-1])
    mid_seq, mid_starts = bf.interleave_mates(r1[::-1], r2[::-1])  # what the buffers in between hold before the kernel ran
    n_pairs = len(pairs)

    def setup(g):
        a, sa = g.late(None, s1, d1), g.late(None, st1.astype(np.uint64), dst1.astype(np.uint64))
        b, sb = g.late(None, s2, d2), g.late(None, st2.astype(np.uint64), dst2.astype(np.uint64))
        out, out_starts = to_device(mid_seq), to_device(mid_starts)
        prob, minc = to_device(np.asarray(case.prob, np.float64)), to_device(np.asarray(case.minc, np.int32))

        def call():
            lib.check(L_.btlbf_interleave_mates(ptr(a), ptr(sa), ptr(b), ptr(sb), n_pairs, ptr(out), ptr(out_starts),
                                                lib.DEVICE, 0, cur(a)))
            return case.m.classifyPairs(out, prob, minc, max_results=1, starts=out_starts, **classify_kw())
        return call

    case.m.setScratchBudget(BUDGETS[budget] * 8192)
    try:
        run_gated("interleave_mates + classify_pairs %s u%d" % (budget, 8 * id_bytes), delay, setup,
                  lambda got, note: check_rows(bf, got, exp, 1, note), monkeypatch, byte)
    finally:
        case.m.setScratchBudget(0)


@pytest.mark.parametrize("byte", POISONS)
def test_mibf_classify_tally(bf, delay, monkeypatch, byte):  # noqa: F811
    """device results that are late, added to running totals that are late as well (they are inputs too)"""
    n_rows, max_results, n_ids = 257, 4, 40
    r, d = tally_results(bf, n_rows, max_results, n_ids, 11), tally_results(bf, n_rows, max_results, n_ids, 12)
    exp = tally_model(*r, n_ids)
    rng = np.random.RandomState(13)
    base = [rng.randint(0, 1000, n).astype(np.uint64) for n in (n_ids, n_ids, 6)]

    def dev(x):
        return [np.ascontiguousarray(x[0]).view(np.int32).reshape(n_rows, max_results, 4)] + [a.view(np.int32) for a in x[1:]]

    def setup(g):
        ins = [g.late(None, a, b) for a, b in zip(dev(r), dev(d))]
        tot = []
        for name, b_ in zip(("best", "any", "totals"), base):
            t, _ = g.alloc(len(b_), np.uint64, name)
            tot.append(g.late(t, b_, b_ + np.uint64(5)))
        return lambda: bf.classify_tally(*ins, n_ids, best=tot[0], any_=tot[1], totals=tot[2])

    def check(got, note):
        for name, g_, b_, e in zip(("best", "any", "totals"), got, base, exp):
            assert_same("%s: %s" % (note, name), g_, b_ + e)

    run_gated("mibf classify_tally", delay, setup, check, monkeypatch, byte)


# ---------------------------------------------------------------------------------------------
# 9. BTLBF_HOST calls on the gated stream: numpy inputs with stream=s; they synchronise before returning
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("path", ["staged", "mailbox"])
def test_host_hash_seqs(bf, delay, oracle, hashes, monkeypatch, byte, path):  # noqa: F811
    """staged: the ragged buffer with `starts`; mailbox: one sequence of 4100 bytes without `starts`"""
    lay = hashes.lay
    if path == "staged":
        buf, kw, w = u8(lay.buf), dict(starts=lay.starts), hashes.win
    else:
        lo, hi = next((lo, hi) for lo, hi in lay.seqs if hi - lo == 4100)
        buf, kw = u8(lay.buf[lo:hi]), {}
        w = oc.Windows(oracle, lay.buf[lo:hi], [(0, hi - lo)], K, H)

    def check(got, note):
        assert_same(note + ": hashes", got[0], w.rows)
        assert_bitmap(note + ": valid_bits", got[1], w.clean, len(buf))

    run_gated("host hash_seqs " + path, delay, lambda g: lambda: bf.hash_seqs(buf, H, K, stream=g.s, **kw), check,
              monkeypatch, byte, host_call=True)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("path", ["staged", "mailbox", "partitioned", "per_thread"])
def test_host_contains_seqs(bf, delay, bitcase, part, monkeypatch, byte, path):  # noqa: F811
    """staged: 300 000 bytes; mailbox: the first 100 reads (15 000 bytes <= 65 536, no `starts`); partitioned: the forced
    partitioned query from host memory; per_thread: the mailbox call on BTLBF_STREAM_PER_THREAD, which is not the gated
    stream -- its outputs are complete on return all the same"""
    c = bitcase
    if path == "partitioned":
        f = bf.BloomFilter(BITS, H, K)
        f.upload(part.body)
        f.setQueryMode("partitioned")
        buf = part.q.cpu().numpy()
        n = buf.size

        def check(got, note):
            assert_bitmap(note + ": hit_bits", got[0], bits_of(part.answer[0], n), n)
            assert_bitmap(note + ": valid_bits", got[1], bits_of(part.answer[1], n), n)
            assert_same(note + ": counts", got[2], part.answer[2])
    else:
        f = c.flt
        n = c.n if path == "staged" else 100 * L
        buf = u8(c.lay.buf)[:n]

        def check(got, note):
            oc.check_query(note, got, n, c.win.clean[:n], c.hit[:n], True, True)

    def setup(g):
        stream = 2 if path == "per_thread" else g.s  # BTLBF_STREAM_PER_THREAD
        return lambda: f.containsSeqs(buf, read_len=L, want_valid=True, want_counts=True, stream=stream)

    run_gated("host containsSeqs " + path, delay, setup, check, monkeypatch, byte, host_call=path != "per_thread")


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("path", ["staged", "mailbox"])
def test_host_min_count_seqs(delay, countcase, monkeypatch, byte, path):
    """45 000 bytes: through the mailbox without `starts`, staged with them"""
    c = countcase
    kw = dict(read_len=L) if path == "mailbox" else dict(starts=(np.arange(301) * L).astype(np.uint64))

    def check(got, note):
        assert_same(note + ": min_out", got[0], c.want_min)
        assert_bitmap(note + ": valid_bits", got[1], c.win.clean, c.n)

    run_gated("host minCountSeqs " + path, delay, lambda g: lambda: c.flt.minCountSeqs(u8(c.lay.buf), stream=g.s, **kw), check,
              monkeypatch, byte, host_call=True)


@pytest.mark.parametrize("byte", POISONS)
def test_host_rank_query(bf, delay, bitcase, monkeypatch, byte):  # noqa: F811
    c = bitcase
    L_, lib = bf._lib.load(), bf._lib
    rs = bf.RankSupport(c.flt)
    bits = np.unpackbits(c.body, bitorder="little")
    csum = np.zeros(BITS + 1, np.uint64)
    csum[1:] = np.cumsum(bits, dtype=np.uint64)
    v = np.random.RandomState(5).randint(0, BITS, 1000).astype(np.uint64)
    pos = v.astype(np.int64)

    def setup(g):
        rank, p_rank = g.reg.alloc(v.size, np.uint64, None, "rank_out")
        bit, p_bit = g.reg.alloc(v.size, np.uint8, None, "bit_out")

        def call():
            lib.check(L_.btlbf_rank_query(rs._h, C.c_void_p(v.ctypes.data), v.size, 0, p_rank, p_bit, lib.HOST,
                                          C.c_void_p(g.s.cuda_stream)))
            return rank, bit
        return call

    def check(got, note):
        assert_same(note + ": rank_out", got[0], csum[pos])
        assert_same(note + ": bit_out", got[1], bits[pos])

    run_gated("host rank_query", delay, setup, check, monkeypatch, byte, host_call=True)


@pytest.mark.parametrize("byte", POISONS)
def test_host_mibf_query(delay, mibfs, monkeypatch, byte):
    c = mibfs[2]

    def check(got, note):
        assert_same(note + ": values", got[0], c.values.astype(c.m.dtype))
        assert_bitmap(note + ": match_bits", got[1], c.match, len(c.q))
        assert_bitmap(note + ": valid_bits", got[2], c.qvalid, len(c.q))
        assert_same(note + ": counts2", got[3], np.array([c.qvalid.sum(), c.match.sum()], np.uint64))

    run_gated("host mibf query_seqs", delay, lambda g: lambda: c.m.query(c.q, max_miss=1, starts=c.qst, want_counts=True, stream=g.s),
              check, monkeypatch, byte, host_call=True)


# host-memory inserts and updates on the gated stream: judged by the body, and by the gate having opened on return (an
# insert that returned before its kernel ran would return before the delay ahead of it had passed).  The inserts, the
# miBF calls and btlbf_rank_query have no mailbox path: their one host path is what runs here.
@pytest.mark.parametrize("path", ["fresh_direct", "fresh_partitioned"])
def test_host_insert_seqs_first_use(bf, delay, bitcase, part, path):  # noqa: F811
    """the first use of a fresh filter -- its lazy clear -- made by a host call on the gated stream"""
    c = bitcase
    buf, want = (u8(c.lay.buf), c.alone) if path == "fresh_direct" else (part.reads.cpu().numpy(), part.body)

    def setup(g):
        f = bf.BloomFilter(BITS, H, K)
        f.setInsertMode("direct" if path == "fresh_direct" else "partitioned")
        f.setProfiling(True)
        return (lambda: f.insertSeqs(buf, read_len=L, stream=g.s)), (lambda: (f.download(), f.getProfile()))

    def check(got, note):
        assert_same(note + ": filter body", got[0], want)
        assert ("insert_apply" in got[1]) == (path == "fresh_partitioned"), (note, got[1])

    run_gated("host insertSeqs " + path, delay, setup, check, host_call=True)


def test_host_counting_insert_seqs(bf, delay, countcase):  # noqa: F811
    c = countcase

    def setup(g):
        f = c.filter(bf)
        return (lambda: f.insertSeqs(u8(c.lay.buf), read_len=L, increment_all=True, stream=g.s)), f.download

    def check(got, note):
        try:
            uo.check_increment_all(got[0], c.all)
        except uo.ContractViolation as e:
            pytest.fail("%s: %s" % (note, e))

    run_gated("host counting insertSeqs incrementAll", delay, setup, check, host_call=True)


@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("op", ["insertIDs", "insertSaturation"])
def test_host_mibf_updates(bf, delay, mibfs, monkeypatch, byte, op):  # noqa: F811
    c = mibfs[2]
    exp, data, counts = c.sat[True]

    def setup(g):
        if op == "insertIDs":
            m = bf.MIBloomFilter(c.f, 2)
            return (lambda: m.insertIDs(c.seq, c.ids, starts=c.starts, stream=g.s)), (lambda: (m.data(), m.counts()))
        m = c.inserted(bf)
        return (lambda: [m.insertSaturation(c.seq, c.ids, starts=c.starts, serial=True, stream=g.s)]), (lambda: (m.data(), m.counts()))

    def check(got, note):
        if op == "insertSaturation":
            assert [got[0][x] for x in ("clean", "found", "mutated", "saturated")] == exp, note
        want_data, want_counts = (c.data1, c.counts1) if op == "insertIDs" else (data, counts)
        assert (got[-1].astype(np.int64) == want_counts).all(), note + ": counts"
        assert (got[-2].astype(np.int64) == want_data).all(), note + ": data"

    run_gated("host mibf " + op, delay, setup, check, monkeypatch, byte, host_call=True)
