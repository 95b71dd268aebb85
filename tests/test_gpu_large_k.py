"""The sequence kernels at the k-mer sizes the API accepts (k up to 32768; spaced seeds up to k = 1024), against the CPU
oracle -- which tests/golden/large_k.json pins to the genuine reference at these sizes -- and the suite's numpy models.
Integer work, every comparison exact.

Thresholds, derived on the host (test_thresholds_are_the_ones_derived_on_the_host: large_k_cases.py from
seq_tile_cap's formula, and the library's planner through btlbf_plan_pass_a), and the tests on either side of them:

  extra staging loop of seq_stage_convert ("large k only")
    256-thread kernels (seq, wide counter, miBF, screen; tile 2048, 3 words per thread): first runs at k = 1011.
      k = 1010 | 1011 in K_LADDER: hash_seqs, direct bit filter; 8-bit counters, wide counters and the screen at 1011
      and above; miBF at 2049.  Up to k = 1025 (1022 for a buffer misaligned by 3) the words that loop converts are
      the image's rounding slack, which no window reads; from k = 1026 (1023) they hold bases of the last windows, so
      1026 is in K_LADDER too.
    pass A (1024 threads, tile 8192, 3 words per thread; the overlapped schedule's 512 staging threads take 6 words
      each: the same 3072 words): first runs at k = 4083, first read by a window at k = 4098 (4095).
      test_pass_a_extra_staging_loop_both_schedules (k = 4100, 512 bins), and every partitioned case at k >= 4194.
  Horner start-up (no positional table): plain ntHash at k > 128 in the direct kernels -- every rung of K_LADDER.
  windows longer than a tile (k >= 2049): rungs 2049 and up.
  count_windows_kernel's chunk of 8192 bytes: k - 1 > 8192 from k = 8194; test_count_windows at 8192 | 8193 | 8194.
  pass A stops fitting the LDS (plain ntHash; the call takes the direct kernels above):
      256 level-0 bins: last k = 13410 (room for the ragged layout's start bitmap, i.e. the overlapped schedule: 11006)
      512 bins:         last k = 10338 (8274)
      1024 bins:        last k = 4194  (2814)
      32 bins (a 2^30-bit filter's own plan): last k = 16098 (13394)
    test_partitioned_on_either_side_of_pass_a (k = last | last + 1 per bin count, the route read from the profile);
    the ragged cases there sit above the start-bitmap limit (plain schedule), test_pass_a_extra_staging_loop_both_schedules
    below it (overlapped schedule with the default scratch, plain with 1 GiB), and
    test_overlapped_schedule_on_either_side_of_the_start_bitmap_limit at k = 8274 | 8275 with 512 bins: the overlapped
    schedule with a window longer than pass A's tile, and the first k that goes without the bitmap.
  read grid (pass A, uniform reads): part_read_grid takes 16 <= L <= 4096 with L >= k where it keeps 5 % more lanes
    busy than plain tiles, whatever k; test_partitioned_read_grid_at_large_k at (k, L) = (1011, 1100) and (4000, 4088)
    with the grid, (4000, 4096) (two reads per tile: no gain) and (4000, 4097) without, as btlbf_plan_read_grid says.  Every other uniform case here has L > 4096.
  AUTO query: the read sampler and the split routes need a batch worth a sweep (4 * 10^6 probes);
    test_auto_query_uniform_reads tiles a few dozen reads to that size on the device and reads the route from the
    profile.
  spaced seeds and the LDS (k = 1024: 131200 bytes of positional table): test_spaced_lds_* -- 14008 don't-care
    positions in all fit (163840 bytes with the static 1536), 14009 do not and are refused by setSpacedSeeds.

K_LADDER = 129, 1010, 1011, 1026, 2049, 4097, 32768 plus the two k on either side of each pass-A boundary."""
import ctypes as C

import numpy as np
import pytest

import large_k_cases as lk
import mibf_classify_model as cm
import mibf_model as mm
import wide_counter_model as wm
from conftest import load_golden
from poison import POISONS, assert_bitmap, assert_same, check_guards, poisoned_outputs

gpu = pytest.mark.gpu

PASS_A_LAST = {256: 13410, 512: 10338, 1024: 4194}       # last k pass A fits, per level-0 bins
PASS_A_LAST_OVERLAPPED = {256: 11006, 512: 8274, 1024: 2814}  # ... with room for the ragged layout's start bitmap
SPLIT_BITS = {256: "3", 512: "2", 1024: "1"}  # BTLBF_SPLIT_BITS that gives a 2^30-bit filter (2048 segments) these bins
K_LADDER = sorted(set(lk.K_BASE) | {1026} | {k + d for k in PASS_A_LAST.values() for d in (0, 1)})
H = 3
SIZES3 = (1 << 16, 100000, (1 << 32) + (1 << 20) + 64)
SPACED_KS = [129, 512, 1024]
LDS_BYTES, LDS_STATIC = 160 * 1024, 1536  # csrc/internal.hpp kLdsPerWorkgroup, kSeqStaticLds


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    return m


def test_thresholds_are_the_ones_derived_on_the_host(lib):
    """CPU: the constants of this file against seq_tile_cap's formula and the library's planner"""
    assert lk.first_k_with_extra_staging(256) == 1011 and lk.first_k_with_extra_staging(1024) == 4083
    # ... and the first k at which a window reads what that loop staged, for an aligned buffer and one misaligned by 3
    assert [lk.first_k_reading_the_extra_words(256, m) for m in (0, 3)] == [1026, 1023]
    assert [lk.first_k_reading_the_extra_words(1024, m) for m in (0, 3)] == [4098, 4095]
    assert 1026 in K_LADDER and 4100 >= 4098
    # the overlapped schedule's 512 stagers convert 6 words each (kStageKW = 20): as many words as 1024 x 3
    assert (20 // 4 + 1) * 512 == (8 // 4 + 1) * 1024
    b = lk.pass_a_boundaries(lib)
    assert {bins: v[0] for bins, v in b.items()} == PASS_A_LAST
    assert {bins: v[1] for bins, v in b.items()} == PASS_A_LAST_OVERLAPPED
    assert sorted(lk.k_ladder(lib) + [1026]) == K_LADDER
    # 32 bins, what a 2^30-bit filter plans by itself (the figures include/btlbf.h and DESIGN.md give)
    assert lk.last_k(lambda k: lk.plan_pass_a(lib, k, H, 32)[0] == 1, lo=129) == 16098
    assert lk.last_k(lambda k: lk.plan_pass_a(lib, k, H, 32)[3] != 0, lo=129) == 13394
    # pass A's dynamic LDS at the last k that fits is within 16 bytes (the image's rounding) of the budget
    for bins, k in PASS_A_LAST.items():
        assert 160 * 1024 - 1664 - 16 < lk.plan_pass_a(lib, k, H, bins)[1] <= 160 * 1024 - 1664
    assert 4083 <= 4100 <= PASS_A_LAST_OVERLAPPED[512]


# ---- helpers ---------------------------------------------------------------------------------------------------
def dev(a, mis=0):
    """a host byte string / uint8 array on the GPU, its base pointer misaligned by `mis` bytes"""
    import torch

    a = np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, np.uint8)
    t = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
    t[mis:mis + a.size] = torch.from_numpy(a.copy()).cuda()
    out = t[mis:mis + a.size]
    assert out.data_ptr() % 4 == mis % 4
    return out


def dev_starts(st):
    import torch

    return torch.from_numpy(st.astype(np.int64)).cuda()


def host(x):
    return x if isinstance(x, np.ndarray) else x.contiguous().cpu().numpy()


def u64(x):
    return np.ascontiguousarray(host(x)).view(np.uint64)


def variants(b, mems=("host", 0, 1, 3)):
    """(label, seq, layout keywords) of a buffer in host memory and on the device at the given misalignments"""
    for m in mems:
        if m == "host":
            yield "host", np.frombuffer(b.buf, np.uint8), b.kw()
        else:
            yield "dev+%d" % m, dev(b.buf, m), dict(starts=None if b.starts is None else dev_starts(b.starts), read_len=b.read_len)


_cache = {}


def buffers(k):
    """the buffers of one k: ragged, uniform with read_len k and k + 1"""
    if k not in _cache:
        _cache[k] = (lk.ragged_buffer(k), lk.uniform_buffer(k, k), lk.uniform_buffer(k, k + 1))
        r = _cache[k][0]
        assert r.n % 64 != 0 and r.n <= 9 * k + 6300
    return _cache[k]


_wcache = {}


def windows(oracle, b, k, h=H, seeds=None):
    key = (id(b), k, h, tuple(seeds or ()))
    if key not in _wcache:
        _wcache[key] = lk.Windows(oracle, b, k, h, seeds)
    return _wcache[key]


def check_hash_output(name, got, b, w, seeds=False):
    hv, valid = got[0], got[1]
    assert_bitmap(name + " valid_bits", valid, w.clean, b.n)
    assert_same(name + " hashes", u64(hv), w.rows)
    if seeds:
        assert_same(name + " strand_bits", u64(got[2]), w.strand)


# ---- 1. hash_seqs, plain ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", K_LADDER)
def test_hash_seqs_plain(bf, oracle, k):
    for b in buffers(k):
        w = windows(oracle, b, k)
        assert w.idx.size > 0
        for label, seq, kw in variants(b, ("host", 0, 1, 3) if b.kind == "ragged" else ("host", 1)):
            check_hash_output("k=%d %s %s" % (k, b.kind, label), bf.hash_seqs(seq, H, k, **kw), b, w)


@gpu
@pytest.mark.parametrize("case", [c for c in lk.golden_cases() if c["kind"] != "kmer"], ids=lambda c: c["name"])
def test_hash_streams_against_the_reference_digests(bf, case):
    """the inputs of tests/golden/large_k.json through the GPU: positions and values hash to the reference's"""
    s = np.frombuffer(lk.build_input(case["input"]), np.uint8)
    k = case["k"]
    if case["kind"] == "nthash":
        hv, valid = bf.hash_seqs(s, case["h"], k)
        st = None
    else:
        sd = case["seeds"]
        hv, valid, st = bf.sthash_seqs(s, lk.make_seeds(sd["seed"], k, sd["n"], sd["p_one"]), case["h2"], k)
    v = bf.bits_to_bool(valid, s.size)
    pos = np.flatnonzero(v)
    got = dict(pos=pos, hashes=u64(hv)[pos])
    if st is not None:
        m = got["hashes"].shape[1]
        got["strand"] = ((u64(st)[pos][:, None] >> np.arange(m, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    assert lk.digest_case(got) == load_golden(lk.GOLDEN_FILE)[case["name"]]["expected"]


# ---- 2. sthash_seqs --------------------------------------------------------------------------------------------
def spaced_seeds(k):
    return lk.make_seeds(5000 + k, k, 3)


@gpu
@pytest.mark.parametrize("k", SPACED_KS)
def test_sthash_seqs(bf, oracle, k):
    seeds = spaced_seeds(k)
    for b in (buffers(k)[0], buffers(k)[2]):
        w = windows(oracle, b, k, 3, seeds)
        assert w.idx.size > 0 and w.strand.any()
        for label, seq, kw in variants(b, ("host", 0, 3)):
            check_hash_output("k=%d %s %s" % (k, b.kind, label), bf.sthash_seqs(seq, seeds, 1, k, **kw), b, w, seeds=True)


# ---- 3. direct bit filter (and 12. count_per_seq) --------------------------------------------------------------
def check_body(bf, f, exp, bits, name):
    if bits <= 1 << 24:
        assert_same(name + " body", f.download(), exp)
    else:  # 512 MiB: by digest and population, computed where the array lies
        assert f.digest() == bf.engine.body_digest(exp), name
        assert f.getPop() == int(np.unpackbits(exp[np.flatnonzero(exp)]).sum()), name


def per_seq_counts(b, k, hit, clean):
    hits = np.array([hit[lo:max(hi - k + 1, lo)].sum() for lo, hi in b.seqs], np.uint32)
    valid = np.array([clean[lo:max(hi - k + 1, lo)].sum() for lo, hi in b.seqs], np.uint32)
    return hits, valid


@gpu
@pytest.mark.parametrize("bits", SIZES3)
@pytest.mark.parametrize("k", K_LADDER)
def test_direct_bit_filter(bf, oracle, k, bits):
    ragged, uk, uk1 = buffers(k)
    wr, wk, wk1 = (windows(oracle, b, k) for b in (ragged, uk, uk1))
    f = bf.BloomFilter(bits, H, k)
    f.setInsertMode("direct")
    f.setQueryMode("direct")
    body = np.zeros(bits // 8, np.uint8)
    name = "k=%d bits=%d" % (k, bits)
    # insertSeqs: the ragged buffer (device, misaligned) and the reads of k bases (host)
    f.insertSeqs(dev(ragged.buf, 1), starts=dev_starts(ragged.starts))
    f.insertSeqs(np.frombuffer(uk.buf, np.uint8), read_len=k)
    oracle.bf_insert(body, bits, H, wr.crows)
    oracle.bf_insert(body, bits, H, wk.crows)
    check_body(bf, f, body, bits, name + " insertSeqs")
    # containsSeqs with counts: what was inserted, and reads that were not
    for b, w, mems in ((ragged, wr, ("host", 3)), (uk1, wk1, (0,))):
        hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, bits, H, w.crows).astype(bool))
        assert b is not ragged or hit[w.idx].all()
        for label, seq, kw in variants(b, mems):
            gh, gv, gc = f.containsSeqs(seq, want_counts=True, **kw)
            assert_bitmap(name + " contains hit " + label, gh, hit, b.n)
            assert_bitmap(name + " contains valid " + label, gv, w.clean, b.n)
            assert_same(name + " contains counts " + label, gc, np.array([w.clean.sum(), hit.sum()], np.uint64))
            if k == 2049:  # 12. count_per_seq over these bitmaps
                ph, pv = bf.count_per_seq(gh, gv, b.n, k, starts=kw["starts"], read_len=kw["read_len"])
                eh, ev = per_seq_counts(b, k, hit, w.clean)
                assert_same(name + " count_per_seq hits " + label, np.ascontiguousarray(host(ph)).view(np.uint32), eh)
                assert_same(name + " count_per_seq valid " + label, np.ascontiguousarray(host(pv)).view(np.uint32), ev)
    # insertAndCheckSeqs: the reads of k + 1 bases, twice
    hit, amb = lk.insert_and_check_expectation(body, bits, wk1, uk1.n)
    gh, gv, gc = f.insertAndCheckSeqs(dev(uk1.buf, 3), read_len=k + 1, want_counts=True)
    got = bf.bits_to_bool(host(gh), uk1.n)
    want = np.where(amb, got, hit)
    assert amb.sum() * 4 < wk1.idx.size
    assert_bitmap(name + " insertAndCheck hit", gh, want, uk1.n)
    assert_bitmap(name + " insertAndCheck valid", gv, wk1.clean, uk1.n)
    assert_same(name + " insertAndCheck counts", gc, np.array([wk1.clean.sum(), want.sum()], np.uint64))
    oracle.bf_insert(body, bits, H, wk1.crows)
    check_body(bf, f, body, bits, name + " insertAndCheckSeqs")
    gh, gv, _ = f.insertAndCheckSeqs(np.frombuffer(uk1.buf, np.uint8), read_len=k + 1)
    assert_bitmap(name + " insertAndCheck again", gh, wk1.clean, uk1.n)


# ---- 4. 8-bit counting filter ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1011, 4097])
def test_counting8(bf, oracle, k):
    ragged, uk, uk1 = buffers(k)
    f = bf.CountingBloomFilter(1 << 16, H, k, 2)
    f.setInsertMode("direct")
    f.setQueryMode("direct")
    c = np.zeros(f.size(), np.uint8)
    for b, (label, seq, kw) in ((ragged, next(variants(ragged, (1,)))), (ragged, next(variants(ragged, ("host",)))),
                                (uk1, next(variants(uk1, (0,))))):
        f.insertSeqs(seq, increment_all=True, **kw)
        oracle.cbf_increment_all(c, H, windows(oracle, b, k).crows)
    assert_same("k=%d counters" % k, f.download(), c)
    assert c.max() >= 2
    for b in (ragged, uk, uk1):
        w = windows(oracle, b, k)
        mn = lk.spread(b.n, w.idx, oracle.cbf_query(c, H, 2, w.crows)[0], np.uint8)
        for label, seq, kw in variants(b, ("host", 3)):
            gm, gv = f.minCountSeqs(seq, **kw)
            assert_same("k=%d %s %s min counts" % (k, b.kind, label), gm, mn)
            assert_bitmap("k=%d %s %s valid" % (k, b.kind, label), gv, w.clean, b.n)


# ---- 5. wide counters ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bits", [16, 64])
@pytest.mark.parametrize("k", [1011, 2049])
def test_wide_counters(bf, oracle, k, bits):
    ragged, uk, uk1 = buffers(k)
    nbytes = 1 << 15
    f = bf.CountingBloomFilter(nbytes, H, k, 2, counter_bits=bits)
    model = wm.WideCBF(bits, nbytes, H, k, 2)
    assert f.size() == model.size
    before = np.array(model.c, np.uint64)
    pos = []
    for b, (label, seq, kw) in ((ragged, next(variants(ragged, (3,)))), (ragged, next(variants(ragged, ("host",)))),
                                (uk1, next(variants(uk1, (0,))))):
        f.insertSeqs(seq, increment_all=True, **kw)
        pos.append((windows(oracle, b, k).crows % np.uint64(model.size)).ravel())
    after = wm.increment_all_exact(before, np.concatenate(pos), model.max)
    wm.check_increment_all(f.counters(), after)
    model.c = [int(x) for x in after]
    for b in (ragged, uk):
        w = windows(oracle, b, k)
        mn = lk.spread(b.n, w.idx, [model.min_count(r) for r in w.crows], f.dtype)
        for label, seq, kw in variants(b, ("host", 1)):
            gm, gv = f.minCountSeqs(seq, **kw)
            assert_same("k=%d u%d %s %s min counts" % (k, bits, b.kind, label), np.ascontiguousarray(host(gm)).view(f.dtype), mn)
            assert_bitmap("k=%d u%d %s %s valid" % (k, bits, b.kind, label), gv, w.clean, b.n)


# ---- 6. partitioned pipeline -----------------------------------------------------------------------------------
PBITS = 1 << 30


def partitioned_round(bf, oracle, k, b, scratch=0, mems=(0,)):
    """insert `b` into a fresh 2^30-bit filter in partitioned mode and query it there -> the profile of the insert;
    body (digest, population) and query bitmaps against the oracle"""
    w = windows(oracle, b, k)
    body = np.zeros(PBITS // 8, np.uint8)
    oracle.bf_insert(body, PBITS, H, w.crows)
    prof = None
    for label, seq, kw in variants(b, mems):
        f = bf.BloomFilter(PBITS, H, k)
        f.setInsertMode("partitioned", scratch)
        f.setQueryMode("partitioned")
        f.setProfiling(True)
        f.insertSeqs(seq, **kw)
        name = "k=%d %s %s" % (k, b.kind, label)
        assert f.digest() == bf.engine.body_digest(body), name
        assert f.getPop() == oracle.bf_popcount(body, PBITS), name
        prof = f.getProfile()
        # a query of the inserted buffer with one base of every fourth sequence changed: hits and misses
        q = np.frombuffer(b.buf, np.uint8).copy()
        for lo, hi in b.seqs[::4]:
            if hi - lo >= k:
                q[lo + (hi - lo) // 2] = ord("A") if q[lo + (hi - lo) // 2] != ord("A") else ord("C")
        qb = lk.Buf([q[lo:hi].tobytes() for lo, hi in b.seqs], b.kind)
        qw = lk.Windows(oracle, qb, k, H)
        hit = lk.spread(qb.n, qw.idx, oracle.bf_contains(body, PBITS, H, qw.crows).astype(bool))
        assert hit.any() and (qw.clean & ~hit).any()
        qs = dev(qb.buf, 0) if label != "host" else np.frombuffer(qb.buf, np.uint8)
        gh, gv, gc = f.containsSeqs(qs, want_counts=True, **kw)
        assert_bitmap(name + " query hit", gh, hit, qb.n)
        assert_bitmap(name + " query valid", gv, qw.clean, qb.n)
        assert_same(name + " query counts", gc, np.array([qw.clean.sum(), hit.sum()], np.uint64))
        qprof = f.getProfile()
        assert ("query_hash" in qprof) == ("insert_hash" in prof), (name, prof, qprof)
    return prof


@gpu
@pytest.mark.parametrize("side", ["last", "beyond"])
@pytest.mark.parametrize("bins", [256, 512, 1024])
def test_partitioned_on_either_side_of_pass_a(bf, oracle, monkeypatch, bins, side):
    """k = the last size pass A fits with `bins` level-0 bins, and the next: the first runs pass A (insert_hash), the
    second is handed to the direct kernel (insert_direct) -- both give the oracle's filter and answers"""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", SPLIT_BITS[bins])
    k = PASS_A_LAST[bins] + (side == "beyond")
    ragged, uk, uk1 = buffers(k)
    for b in (ragged, uk1):
        prof = partitioned_round(bf, oracle, k, b)
        if side == "last":
            assert prof.get("insert_hash", (0, 0))[1] >= 1 and "insert_direct" not in prof, prof
        else:
            assert "insert_hash" not in prof and prof.get("insert_direct", (0, 0))[1] >= 1, prof


@gpu
@pytest.mark.parametrize("scratch", [0, 1 << 30], ids=["overlapped", "plain"])
def test_pass_a_extra_staging_loop_both_schedules(bf, oracle, monkeypatch, scratch):
    """k = 4100 on 512 bins: pass A runs, its tile image (8192 + k bytes) is more than the 3072 words the threads take
    first, and the ragged layout has its start bitmap -- so the default scratch (>= 2 GiB) runs the overlapped
    schedule's staging and a budget of 1 GiB the plain one"""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", SPLIT_BITS[512])
    k = 4100
    ragged, uk, uk1 = buffers(k)
    for b, mems in ((ragged, (0, 1, "host")), (uk1, (3,))):
        prof = partitioned_round(bf, oracle, k, b, scratch, mems)
        assert prof.get("insert_hash", (0, 0))[1] >= 1 and "insert_direct" not in prof, prof


@gpu
@pytest.mark.parametrize("bins,k", [(512, 8274), (512, 8275)])
def test_overlapped_schedule_on_either_side_of_the_start_bitmap_limit(bf, oracle, monkeypatch, bins, k):
    """ragged input with the default scratch: at k = 8274 pass A still has room for the start bitmap (the overlapped
    schedule, with windows longer than its tile of 8192), at 8275 it runs without; pass A either way"""
    assert k - PASS_A_LAST_OVERLAPPED[bins] in (0, 1) and k > 8192
    monkeypatch.setenv("BTLBF_SPLIT_BITS", SPLIT_BITS[bins])
    prof = partitioned_round(bf, oracle, k, buffers(k)[0], 0, (0, 3))
    assert prof.get("insert_hash", (0, 0))[1] >= 1 and "insert_direct" not in prof, prof


@gpu
@pytest.mark.parametrize("k,L,grid", [(1011, 1100, True), (4000, 4088, True), (4000, 4096, False), (4000, 4097, False)])
def test_partitioned_read_grid_at_large_k(bf, oracle, k, L, grid):
    """uniform reads of at most 4096 bases go through pass A's read grid (a 2^30-bit filter plans 32 level-0 bins)"""
    out = (C.c_uint32 * 4)()
    assert bf._lib.load().btlbf_plan_read_grid(k, H, L, 32, out) == 0
    assert bool(out[0]) == grid, list(out)
    prof = partitioned_round(bf, oracle, k, lk.uniform_buffer(k, L, seed=2), 0, (0, 1))
    assert prof.get("insert_hash", (0, 0))[1] >= 1 and "insert_direct" not in prof, prof


AUTO_H = 8


def auto_period(k, L, cold_every):
    """96 reads of L bases, every cold_every-th of them NOT in the filter; one with an N, one with a raw byte, some lowercase"""
    rng = np.random.RandomState(11000 + k + L + cold_every)
    parts = []
    for i in range(96):
        s = lk.acgt(rng, L)
        if i == 5:
            s[L // 2] = lk.N
        if i == 7:
            s[3] = 4
        if i % 9 == 1:
            s |= 0x20
        parts.append(s.tobytes())
    return lk.Buf(parts, "uniform")


def period_bits(words, first_bit, n):
    """n bits of a bitmap (torch int64 words on the device) from bit first_bit on, as a bool array"""
    w0, w1 = first_bit // 64, (first_bit + n + 63) // 64
    bits = np.unpackbits(host(words[w0:w1]).view(np.uint8), bitorder="little")
    return bits[first_bit - 64 * w0:first_bit - 64 * w0 + n].astype(bool)


@gpu
@pytest.mark.parametrize("k,L,cold_every", [(1024, 1024, 16), (1024, 1025, 3), (4096, 4096, 3), (4096, 4097, 16)])
def test_auto_query_uniform_reads(bf, oracle, k, L, cold_every):
    """AUTO leaves the direct kernel only for a batch worth a sweep of the array (4 * 10^6 probes, worth_sweep): 96
    reads, their answers from the oracle, tiled on the device until the reads that are in the filter alone carry that
    many probes.  One read in 16 foreign: few enough for the partitioned query's fail list (query_hash); one in 3: a
    split route, the foreign reads through the direct kernel (query_direct as well).  The answers equal the direct
    kernel's word for word, and the oracle's in the first and the last period and in the counts."""
    import torch

    b = auto_period(k, L, cold_every)
    w = lk.Windows(oracle, b, k, AUTO_H)
    inserted = (w.idx // L) % cold_every != 0
    body = np.zeros(PBITS // 8, np.uint8)
    oracle.bf_insert(body, PBITS, AUTO_H, w.crows[inserted])
    hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, PBITS, AUTO_H, w.crows).astype(bool))
    assert hit[w.idx][inserted].all() and (w.clean & ~hit).sum() >= 0.9 * (~inserted).sum()
    W = L - k + 1
    n_reads = int(4.4e6 / (W * AUTO_H * (1 - 1 / cold_every))) + 1
    m = -(-n_reads // 96)
    f = bf.BloomFilter(PBITS, AUTO_H, k)
    f.setInsertMode("direct")
    f.insert(w.crows[inserted])
    seq = torch.from_numpy(np.frombuffer(b.buf, np.uint8).copy()).cuda().repeat(m)
    assert seq.numel() == m * b.n
    f.setQueryMode("direct")
    dh, dv, dc = f.containsSeqs(seq, read_len=L, want_counts=True)
    f.setProfiling(True)
    f.setQueryMode("auto")
    ah, av, ac = f.containsSeqs(seq, read_len=L, want_counts=True)
    torch.cuda.synchronize()
    prof = f.getProfile()
    name = "k=%d L=%d 1/%d foreign" % (k, L, cold_every)
    # the read sampler ran (it is timed in the resolve slot) and so did pass A of the partitioned query
    assert prof.get("query_resolve", (0, 0))[1] >= 1 and prof.get("query_hash", (0, 0))[1] >= 1, (name, prof)
    if cold_every == 3:
        assert prof.get("query_direct", (0, 0))[1] >= 1, (name, prof)
    assert torch.equal(ah, dh) and torch.equal(av, dv), name
    want = [m * int(w.clean.sum()), m * int(hit.sum())]
    assert [int(x) for x in ac.tolist()] == want and [int(x) for x in dc.tolist()] == want, (name, ac.tolist(), dc.tolist(), want)
    for first in (0, (m - 1) * b.n):
        assert (period_bits(ah, first, b.n) == hit).all(), (name, first)
        assert (period_bits(av, first, b.n) == w.clean).all(), (name, first)
    del seq, ah, av, dh, dv
    torch.cuda.empty_cache()


# ---- 7. shards -------------------------------------------------------------------------------------------------
@gpu
def test_two_shards(bf, oracle):
    """2 shards at k = 2049 (uniform reads of k + 1: the shard calls take that layout): bodies concatenated and answers
    ANDed are the oracle's single filter (OP_BF_CONTAINS_WIN); btlbf_positions_seqs buckets the oracle's positions"""
    import torch

    from btl_bloomfilter_amd.sharded import HipShardOps

    k, bits, W = 2049, 1 << 22, 2
    b = buffers(k)[2]
    w = windows(oracle, b, k)
    ins = lk.Buf([b.buf[lo:hi] for lo, hi in b.seqs[::2]], "uniform")
    wi = lk.Windows(oracle, ins, k, H)
    body = np.zeros(bits // 8, np.uint8)
    oracle.bf_insert(body, bits, H, wi.crows)
    hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, bits, H, w.crows).astype(bool))
    assert hit.any() and (w.clean & ~hit).any()
    reads, q = dev(ins.buf, 0), dev(b.buf, 0)
    words = (b.n + 63) // 64
    acc, bodies = None, []
    for r in range(W):
        ops = HipShardOps(bits, H, k, r, W, 0)
        ops.insert_seqs(reads, k + 1)
        gh = torch.zeros(words, dtype=torch.int64, device="cuda")
        gv = torch.zeros(words, dtype=torch.int64, device="cuda")
        ops.contains_seqs(q, k + 1, gh, gv)
        assert_bitmap("shard %d valid" % r, gv, w.clean, b.n)
        acc = gh if acc is None else acc & gh
        bodies.append(ops.local_body())
        if r == 0:
            cap = int(w.idx.size * H)
            buckets, tags, counts, valid = ops.positions(q, k + 1, cap, True)
            torch.cuda.synchronize()
            assert_bitmap("positions valid", valid, w.clean, b.n)
            pos = (w.crows % np.uint64(bits)).ravel()
            for g in range(W):
                want = np.sort(pos[(pos // np.uint64(bits // W)) == g] - np.uint64(g * (bits // W)))  # local to the owner
                n = int(counts[g].item())
                assert n == want.size
                assert (np.sort(u64(buckets[g, :n])) == want).all()
        ops.close()
    assert_same("shard bodies", np.concatenate(bodies), body)
    assert_bitmap("AND of the shards' answers", acc, hit, b.n)


# ---- 8. miBF ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cfg", ["nthash_k2049", "spaced_k512"])
def test_mibf(bf, oracle, cfg):
    # (a miBF takes spaced seeds that leave out at most 64 distinct positions, fillers of its offset list included: three
    # seeds of weight 498)
    k, seeds = (2049, None) if cfg == "nthash_k2049" else (512, seeds_with(512, 3, 42))
    h, id_bytes, bits = 3, 2, 1 << 14  # dense: several k-mers per entry, so that saturation has something to do
    b = buffers(k)[0]
    w = windows(oracle, b, k, h, seeds)
    body = np.zeros(bits // 8, np.uint8)
    oracle.bf_insert(body, bits, h, w.crows)
    f = bf.BloomFilter(bits, h, k)
    if seeds:
        f.setSpacedSeeds(seeds, 1)
    f.insertSeqs(np.frombuffer(b.buf, np.uint8), starts=b.starts)
    assert_same(cfg + " stage 1", f.download(), body)
    ranks = mm.Ranks(body, bits)
    wseq = mm.window_seqs(b.n, b.starts)
    ids = (np.arange(len(b.seqs)) % 5 + 1).astype(np.uint32)
    seq, st = np.frombuffer(b.buf, np.uint8), b.starts
    for serial in (True, False):
        m = bf.MIBloomFilter(f, id_bytes)
        assert m.getPop() == ranks.pop
        data, counts = np.zeros(ranks.pop, np.int64), np.zeros(ranks.pop, np.int64)
        if serial:
            m.insertIDs(dev(b.buf, 1), dev_starts(ids).int(), starts=dev_starts(st))
        else:
            m.insertIDs(seq, ids, starts=st)
        mm.insert_ids(data, counts, ranks, w.rows, w.clean, wseq, ids, id_bytes)
        assert_same(cfg + " insertIDs data", m.data().astype(np.int64), data)
        assert_same(cfg + " insertIDs counts", m.counts().astype(np.int64), counts)
        got = m.insertSaturation(seq, ids, starts=st, serial=serial)
        exp = (mm.saturate_serial if serial else mm.saturate_parallel)(data, counts, ranks, w.rows, w.clean, wseq, ids, id_bytes)
        assert [got["clean"], got["found"], got["mutated"], got["saturated"]] == exp and exp[0] == w.idx.size
        assert_same(cfg + " saturation data", m.data().astype(np.int64), data)
        assert_same(cfg + " saturation counts", m.counts().astype(np.int64), counts)
        # query: the inserted buffer and reads that were not inserted
        for qb in (b, buffers(k)[2]):
            qw = windows(oracle, qb, k, h, seeds)
            vals, match = mm.query(data, ranks, qw.rows, qw.clean, 1, bool(seeds))
            for label, qs, kw in variants(qb, ("host", 3)):
                gvals, gm, gv, gc = m.query(qs, max_miss=1, want_counts=True, **kw)
                assert_same(cfg + " query values " + label, np.ascontiguousarray(host(gvals)).view(m.dtype), vals.astype(m.dtype))
                assert_bitmap(cfg + " query match " + label, gm, match, qb.n)
                assert_bitmap(cfg + " query valid " + label, gv, qw.clean, qb.n)
                assert_same(cfg + " query counts " + label, gc, np.array([qw.clean.sum(), match.sum()], np.uint64))
        # classify a handful of reads of the inserted buffer
        reads = [s for s in b.seqs if s[1] - s[0] >= k][:6]
        cb = lk.Buf([b.buf[lo:hi] for lo, hi in reads], "ragged")
        prob, minc = [0.0] + [0.02] * 8, [1] * 9
        hits, n_hits, sat, ev = m.classify(np.frombuffer(cb.buf, np.uint8), prob, minc, max_miss=1 if seeds else 0, starts=cb.starts)
        for i, (lo, hi) in enumerate(cb.seqs):
            rw = lk.Windows(oracle, lk.Buf([cb.buf[lo:hi]], "ragged"), k, h, seeds)
            res, s_, e_ = cm.classify(data, ranks, rw.crows, id_bytes, bool(seeds), prob, minc, max_miss=1 if seeds else 0)
            assert (int(n_hits[i]), int(sat[i]), int(ev[i])) == (len(res), s_, e_), (cfg, i)
            for j, r in enumerate(res[:8]):
                assert tuple(int(x) for x in hits[i, j]) == tuple(int(x) for x in r), (cfg, i, j)


# ---- 9. screenSeqs ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cfg", ["plain_k1011", "plain_k4097", "spaced_k512"])
def test_screen(bf, oracle, cfg):
    import screen_cases as sc

    k = int(cfg.split("k")[1])
    seeds = spaced_seeds(k) if cfg.startswith("spaced") else None
    b = buffers(k)[0]
    w = windows(oracle, b, k, H, seeds)
    wseq = mm.window_seqs(b.n, b.starts)
    bodies = [np.zeros(bits // 8, np.uint8) for bits in SIZES3]
    for j, bits in enumerate(SIZES3):  # filter j holds every sequence i with i % 3 == j
        oracle.bf_insert(bodies[j], bits, H, w.crows[wseq[w.idx] % 3 == j])
    filters = sc.make_filters(bf, bodies, SIZES3, H, k, seeds)
    n_seqs = len(b.seqs)
    hits = np.zeros((n_seqs, 3), np.uint32)
    for j, bits in enumerate(SIZES3):
        hj = oracle.bf_contains(bodies[j], bits, H, w.crows).astype(np.int64)
        hits[:, j] = np.bincount(wseq[w.idx], weights=hj, minlength=n_seqs).astype(np.uint32)
    valid = np.bincount(wseq[w.idx], minlength=n_seqs).astype(np.uint32)
    if not seeds:  # (oracle_counts walks plain ntHash)
        oh, ov = sc.oracle_counts(oracle, [np.frombuffer(b.buf[lo:hi], np.uint8) for lo, hi in b.seqs], bodies, SIZES3, H, k)
        assert (oh == hits).all() and (ov == valid).all()
    seq = np.frombuffer(b.buf, np.uint8)
    eh, ev = sc.existing_path(bf, filters, seq, k, starts=b.starts)
    assert (eh == hits).all() and (ev == valid).all()
    for label, qs, kw in variants(b, ("host", 1)):
        out = bf.screenSeqs(filters, qs, min_fraction=0.5, min_hits=1, **kw)
        gh, gv = sc.host(out[0]).reshape(n_seqs, -1)[:, :3], sc.host(out[1])
        assert_same(cfg + " screen hits " + label, np.ascontiguousarray(gh), hits)
        assert_same(cfg + " screen valid " + label, gv, valid)


# ---- 10. countWindows ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [8192, 8193, 8194, 20000, 32768])
def test_count_windows(bf, oracle, k):
    from test_gpu_mibf_build_file import window_counts

    ragged, uk, uk1 = buffers(k)
    for b in (ragged, uk, uk1, lk.Buf([ragged.buf], "single")):
        a = np.frombuffer(b.buf, np.uint8)
        exp = window_counts(a, k, b.starts, b.read_len)
        assert exp[0] > 0 and exp[1] > 0
        for label, seq, kw in variants(b, ("host", 0, 3)):
            assert bf.countWindows(seq, k, **kw) == exp, (k, b.kind, label)
        if k == 20000:  # the clean count is the number of windows the hash kernel emits
            _, valid = bf.hash_seqs(a, 1, k, **b.kw())
            assert int(bf.bits_to_bool(valid, b.n).sum()) == exp[1]


# ---- 11. raw k-mers --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", [1023, 1024, 1026, 4097, 32768])
def test_raw_kmers(bf, oracle, k):
    """k % 4 = 3, 0, 2, 1, 0; lowercase, U, an invalid byte and a raw byte (large_k_cases.kmer_recipe)"""
    s = lk.build_input(lk.kmer_recipe(4000 + k, k))
    ehv, eok = oracle.kmer_hashes(s, k, H)
    # k-mer 6 has an N in its 2- / 3-base tail: no value at k % 4 = 2 or 3 (valid = 0), a value otherwise
    assert eok.tolist() == [1] * 6 + [int(k % 4 in (0, 1)), 1]
    golden = load_golden(lk.GOLDEN_FILE).get("kmer_k%d" % k)
    if golden:
        assert lk.digest_case(dict(pos=np.flatnonzero(eok), hashes=ehv[np.flatnonzero(eok)])) == golden["expected"]
    hv, ok = bf.hash_kmers(s, H, k)
    assert_same("k=%d valid" % k, ok, eok)
    assert_same("k=%d hashes" % k, hv[eok == 1], ehv[eok == 1])
    bits = 1 << 20
    f = bf.KmerBloomFilter(bits, H, k)
    body = np.zeros(bits // 8, np.uint8)
    a = np.frombuffer(s, np.uint8)
    f.insertKmers(a[: 4 * k])
    f.insertKmers(dev(a[6 * k: 7 * k], 3))  # the k-mer that may have no value: then nothing is inserted for it
    oracle.bf_insert(body, bits, H, ehv[[0, 1, 2, 3, 6]][eok[[0, 1, 2, 3, 6]] == 1])
    assert_same("k=%d body" % k, f.download(), body)
    want = oracle.bf_contains(body, bits, H, ehv) & eok
    assert_same("k=%d containsKmers host" % k, f.containsKmers(a), want)
    assert_same("k=%d containsKmers device" % k, f.containsKmers(dev(a, 1)), want)
    assert want.tolist() == [1, 1, 1, 1, 0, 0, int(eok[6]), 0]


# ---- refusals --------------------------------------------------------------------------------------------------
@gpu
def test_k_beyond_the_accepted_range_is_refused(bf):
    from btl_bloomfilter_amd._lib import EINVAL, BtlbfError

    s = np.frombuffer(b"ACGT" * 16384, np.uint8)
    calls = [lambda: bf.BloomFilter(1 << 16, 3, 32769), lambda: bf.CountingBloomFilter(1 << 16, 3, 32769),
             lambda: bf.CountingBloomFilter(1 << 16, 3, 32769, counter_bits=32),
             lambda: bf.BloomFilter.shard(1 << 16, 0, 2, 3, 32769), lambda: bf.hash_seqs(s, 3, 32769),
             lambda: bf.hash_kmers(s, 3, 32769),
             lambda: bf.sthash_seqs(s[:1025], ["1" * 1025], 1, 1025),
             lambda: bf.BloomFilter(1 << 16, 1, 1025).setSpacedSeeds(["1" * 1025], 1)]
    for i, call in enumerate(calls):
        with pytest.raises(BtlbfError) as e:
            call()
        assert e.value.code == EINVAL, (i, str(e.value))
    bf.BloomFilter(1 << 16, 3, 32768).close()
    bf.BloomFilter(1 << 16, 1, 1024).setSpacedSeeds(["1" * 1024], 1)


@gpu
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("family", ["hash", "sthash", "contains", "insert_and_check", "min_count8", "min_count_wide", "mibf_query",
                                    "screen", "count_per_seq"])
def test_outputs_fully_written_at_k_2049(bf, oracle, monkeypatch, byte, family):
    """every byte of every output is stored by the call: dirty, guarded outputs (tests/poison.py), device memory"""
    k = 2049 if family != "sthash" else 1024  # (spaced seeds end at 1024)
    b = buffers(k)[0]
    seeds = spaced_seeds(k) if family == "sthash" else None
    w = windows(oracle, b, k, H, seeds)
    seq, st = dev(b.buf, 1), dev_starts(b.starts)
    bits = 1 << 16
    body = np.zeros(bits // 8, np.uint8)
    oracle.bf_insert(body, bits, H, w.crows[::2])
    hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, bits, H, w.crows).astype(bool))
    name = "%s 0x%02x" % (family, byte)
    if family in ("contains", "insert_and_check", "count_per_seq", "mibf_query", "screen"):
        f = bf.BloomFilter(bits, H, k)
        f.upload(body)
    if family == "mibf_query":
        m = bf.MIBloomFilter(f, 2)
        ranks = mm.Ranks(body, bits)
        data = np.arange(1, ranks.pop + 1, dtype=np.int64) % 100 + 1
        m.upload(data.astype(m.dtype))
    if family == "count_per_seq":
        gh, gv, _ = f.containsSeqs(seq, starts=st)
    if family.startswith("min_count"):
        wide = family.endswith("wide")
        c = bf.CountingBloomFilter(1 << 15, H, k, 1, counter_bits=32 if wide else 8)
        c.insertSeqs(seq, starts=st, increment_all=True)
        cnt = c.counters().astype(np.uint64)
        mn = lk.spread(b.n, w.idx, cnt[(w.crows % np.uint64(c.size())).astype(np.int64)].min(axis=1), c.dtype)
    poisoned_outputs(monkeypatch, byte)
    if family == "hash":
        check_hash_output(name, bf.hash_seqs(seq, H, k, starts=st), b, w)
    elif family == "sthash":
        check_hash_output(name, bf.sthash_seqs(seq, seeds, 1, k, starts=st), b, w, seeds=True)
    elif family == "contains":
        gh, gv, gc = f.containsSeqs(seq, starts=st, want_counts=True)
        assert_bitmap(name + " hit", gh, hit, b.n)
        assert_bitmap(name + " valid", gv, w.clean, b.n)
        assert_same(name + " counts", gc, np.array([w.clean.sum(), hit.sum()], np.uint64))
    elif family == "insert_and_check":
        want, amb = lk.insert_and_check_expectation(body, bits, w, b.n)
        gh, gv, gc = f.insertAndCheckSeqs(seq, starts=st, want_counts=True)
        want = np.where(amb, bf.bits_to_bool(host(gh), b.n), want)
        assert_bitmap(name + " hit", gh, want, b.n)
        assert_bitmap(name + " valid", gv, w.clean, b.n)
        assert_same(name + " counts", gc, np.array([w.clean.sum(), want.sum()], np.uint64))
    elif family.startswith("min_count"):
        gm, gv = c.minCountSeqs(seq, starts=st)
        assert_same(name + " min counts", np.ascontiguousarray(host(gm)).view(c.dtype), mn)
        assert_bitmap(name + " valid", gv, w.clean, b.n)
    elif family == "mibf_query":
        vals, match = mm.query(data, ranks, w.rows, w.clean, 0, False)
        gvals, gm, gv, gc = m.query(seq, starts=st, want_counts=True)
        assert_same(name + " values", np.ascontiguousarray(host(gvals)).view(m.dtype), vals.astype(m.dtype))
        assert_bitmap(name + " match", gm, match, b.n)
        assert_bitmap(name + " valid", gv, w.clean, b.n)
        assert_same(name + " counts", gc, np.array([w.clean.sum(), match.sum()], np.uint64))
    elif family == "screen":
        import screen_cases as sc

        wseq = mm.window_seqs(b.n, b.starts)
        out = bf.screenSeqs([f], seq, starts=st, min_fraction=0.0, min_hits=1)
        n_seqs = len(b.seqs)
        eh = np.bincount(wseq[w.idx], weights=hit[w.idx].astype(np.int64), minlength=n_seqs).astype(np.uint32)
        ev = np.bincount(wseq[w.idx], minlength=n_seqs).astype(np.uint32)
        assert_same(name + " hits", sc.host(out[0]).reshape(n_seqs, -1)[:, 0].copy(), eh)
        assert_same(name + " valid", sc.host(out[1]), ev)
    elif family == "count_per_seq":
        ph, pv = bf.count_per_seq(gh, gv, b.n, k, starts=st)
        eh, ev = per_seq_counts(b, k, hit, w.clean)
        assert_same(name + " hits", np.ascontiguousarray(host(ph)).view(np.uint32), eh)
        assert_same(name + " valid", np.ascontiguousarray(host(pv)).view(np.uint32), ev)
    check_guards()


@gpu
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("family", ["partitioned_ragged", "partitioned_uniform", "shards", "raw_kmers", "mibf_classify"])
def test_outputs_fully_written_other_routes_at_k_2049(bf, oracle, monkeypatch, byte, family):
    """the same for the routes that are no single direct launch: the partitioned query (its bitmaps are written by pass A
    and refined in place), the shard calls, the raw k-mer calls and the miBF's classify"""
    import torch

    from btl_bloomfilter_amd import _lib

    k = 2049
    name = "%s 0x%02x" % (family, byte)
    if family.startswith("partitioned"):
        b = buffers(k)[0] if family.endswith("ragged") else buffers(k)[2]
        w = windows(oracle, b, k)
        body = np.zeros(PBITS // 8, np.uint8)
        oracle.bf_insert(body, PBITS, H, w.crows[::2])
        hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, PBITS, H, w.crows).astype(bool))
        assert hit.any() and (w.clean & ~hit).any()
        f = bf.BloomFilter(PBITS, H, k)
        f.setInsertMode("direct")
        f.insert(w.crows[::2])
        f.setQueryMode("partitioned")
        f.setProfiling(True)
        seq = dev(b.buf, 1)
        kw = dict(starts=None if b.starts is None else dev_starts(b.starts), read_len=b.read_len)
        poisoned_outputs(monkeypatch, byte)
        for wv, wc in ((True, True), (False, False)):
            gh, gv, gc = f.containsSeqs(seq, want_valid=wv, want_counts=wc, **kw)
            assert_bitmap(name + " hit", gh, hit, b.n)
            if wv:
                assert_bitmap(name + " valid", gv, w.clean, b.n)
            if wc:
                assert_same(name + " counts", gc, np.array([w.clean.sum(), hit.sum()], np.uint64))
            prof = f.getProfile()
            assert prof.get("query_hash", (0, 0))[1] >= 1, prof  # pass A answered, not the direct kernel
        check_guards()
    elif family == "shards":
        from btl_bloomfilter_amd.sharded import HipShardOps, _ptr
        from poison import Poison

        bits, W = 1 << 22, 2
        b = buffers(k)[2]
        w = windows(oracle, b, k)
        ins = lk.Buf([b.buf[lo:hi] for lo, hi in b.seqs[::2]], "uniform")
        body = np.zeros(bits // 8, np.uint8)
        oracle.bf_insert(body, bits, H, lk.Windows(oracle, ins, k, H).crows)
        hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, bits, H, w.crows).astype(bool))
        reads, q = dev(ins.buf, 0), dev(b.buf, 0)
        words, cap = (b.n + 63) // 64, int(w.idx.size * H)
        pos = (w.crows % np.uint64(bits)).ravel()
        reg = Poison(byte)
        acc = np.ones(b.n, bool)
        for r in range(W):
            ops = HipShardOps(bits, H, k, r, W, 0)
            ops.insert_seqs(reads, k + 1)
            gh, _ = reg.alloc(words, np.int64, device="cuda", name="shard hit")
            gv, _ = reg.alloc(words, np.int64, device="cuda", name="shard valid")
            ops.contains_seqs(q, k + 1, gh, gv)
            assert_bitmap(name + " shard %d valid" % r, gv, w.clean, b.n)
            g = np.unpackbits(host(gh).view(np.uint8), bitorder="little")
            assert not g[b.n:].any(), "bits beyond the buffer"
            acc &= g[: b.n].astype(bool)
            buckets, _ = reg.alloc((W, cap), np.int64, device="cuda", name="buckets")
            tags, _ = reg.alloc((W, cap), np.int64, device="cuda", name="tags")
            pv, _ = reg.alloc(words, np.int64, device="cuda", name="positions valid")
            counts = torch.zeros(W, dtype=torch.int64, device="cuda")
            _lib.check(ops.L.btlbf_positions_seqs(ops.f, _ptr(q), q.numel(), C.byref(ops._lay(k + 1)), W, _ptr(buckets), _ptr(tags),
                                                  cap, _ptr(counts), _ptr(pv), ops._sp()))
            torch.cuda.synchronize()
            assert_bitmap(name + " positions valid", pv, w.clean, b.n)
            for o in range(W):
                want = np.sort(pos[(pos // np.uint64(bits // W)) == o] - np.uint64(o * (bits // W)))
                n = int(counts[o].item())
                assert n == want.size and (np.sort(u64(buckets[o, :n])) == want).all(), (name, r, o)
            ops.close()
        assert (acc == hit).all(), name
        reg.check_guards()
    elif family == "raw_kmers":
        s = np.frombuffer(lk.build_input(lk.kmer_recipe(4000 + k, k)), np.uint8)
        ehv, eok = oracle.kmer_hashes(s.tobytes(), k, H)
        assert eok.all()  # (k % 4 == 1: every k-mer has a value, so every row is compared)
        f = bf.KmerBloomFilter(1 << 20, H, k)
        f.insertKmers(s[: 4 * k])
        body = np.zeros((1 << 20) // 8, np.uint8)
        oracle.bf_insert(body, 1 << 20, H, ehv[:4])
        want = oracle.bf_contains(body, 1 << 20, H, ehv)
        reg = poisoned_outputs(monkeypatch, byte)
        hv, p_hv = reg.alloc((8, H), np.uint64, name="hash_kmers rows")
        ok, p_ok = reg.alloc(8, np.uint8, name="hash_kmers valid")
        _lib.check(_lib.load().btlbf_hash_kmers(k, H, C.c_void_p(s.ctypes.data), 8, p_hv, p_ok, _lib.HOST, 0, None))
        assert_same(name + " hash_kmers rows", hv, ehv)
        assert_same(name + " hash_kmers valid", ok, eok)
        assert_same(name + " containsKmers host", f.containsKmers(s), want)
        assert_same(name + " containsKmers device", f.containsKmers(dev(s, 3)), want)
        check_guards()
    else:
        bits = 1 << 14
        b = buffers(k)[0]
        w = windows(oracle, b, k)
        body = np.zeros(bits // 8, np.uint8)
        oracle.bf_insert(body, bits, H, w.crows)
        f = bf.BloomFilter(bits, H, k)
        f.upload(body)
        ranks = mm.Ranks(body, bits)
        m = bf.MIBloomFilter(f, 2)
        data = np.arange(ranks.pop, dtype=np.int64) % 5 + 1
        m.upload(data.astype(m.dtype))
        reads = [s for s in b.seqs if s[1] - s[0] >= k][:5] + [(0, 0)]
        cb = lk.Buf([b.buf[lo:hi] for lo, hi in reads], "ragged")
        prob, minc = [0.0] + [0.02] * 8, [1] * 9
        exp = np.zeros((len(reads), 8), bf.engine.HIT_DTYPE)
        counts = np.zeros((3, len(reads)), np.uint32)
        for i, (lo, hi) in enumerate(cb.seqs):
            rw = lk.Windows(oracle, lk.Buf([cb.buf[lo:hi]], "ragged"), k, H)
            res, s_, e_ = cm.classify(data, ranks, rw.crows, 2, False, prob, minc)
            counts[:, i] = (len(res), s_, e_)
            for j, r in enumerate(res[:8]):
                exp[i, j] = tuple(int(x) for x in r)
        assert counts[0].any()
        poisoned_outputs(monkeypatch, byte)
        gw, gn, gs, ge = m.classify(dev(cb.buf, 1), prob, minc, starts=dev_starts(cb.starts))
        assert_same(name + " hits", np.ascontiguousarray(host(gw)).view(np.uint32), exp.view(np.uint32).reshape(len(reads), 8, 4))
        for tag, got, want in zip(("n_hits", "sat_count", "eval_count"), (gn, gs, ge), counts):
            assert_same(name + " " + tag, np.ascontiguousarray(host(got)).view(np.uint32), want)
        check_guards()


# ---- C. spaced seeds and the LDS -------------------------------------------------------------------------------
def lds_need(k, n_dontcare, n_distinct):
    """bytes of LDS per workgroup a direct sequence kernel needs with spaced seeds (csrc/internal.hpp seq_lds_dyn +
    kSeqStaticLds): tile image, positional table of k + 1 rows, the seeds' don't-care lists (2 bytes per entry), the
    union list (4 bytes per distinct offset, only when there are at most 64)"""
    r16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    return lk.tile_cap(2048, k) + (k + 1) * 128 + r16(2 * n_dontcare) + (r16(4 * n_distinct) if n_distinct <= 64 else 0) + LDS_STATIC


def seeds_with(k, n_seeds, n_dontcare):
    """n_seeds seeds of k characters, first and last 1, with n_dontcare zeros in all, spread as evenly as they go"""
    rng = np.random.RandomState(n_dontcare)
    out = []
    for j in range(n_seeds):
        z = n_dontcare // n_seeds + (j < n_dontcare % n_seeds)
        assert z <= k - 2
        s = np.ones(k, np.uint8)
        s[1 + rng.choice(k - 2, z, replace=False)] = 0
        out.append("".join("01"[c] for c in s))
    return out


LDS_FIT = 14008  # don't-care positions of 16 seeds at k = 1024 that still fit: lds_need(1024, 14008, >64) == 163840


def plan_spaced(lib, k, seeds):
    arr = (C.c_char_p * len(seeds))(*[s.encode() for s in seeds])
    out = (C.c_uint32 * 2)()
    rc = lib.btlbf_plan_spaced_lds(k, arr, len(seeds), 1, out)
    return rc, tuple(out), lib.btlbf_last_error().decode()


def test_spaced_lds_limit_by_host_arithmetic(lib):
    """CPU: the library's refusal is decided where lds_need says, before any device call (this test has no GPU)"""
    assert lds_need(1024, LDS_FIT, 1000) == LDS_BYTES and lds_need(1024, LDS_FIT + 1, 1000) > LDS_BYTES
    rc, out, _ = plan_spaced(lib, 1024, seeds_with(1024, 16, LDS_FIT))
    assert rc == 0 and out == (LDS_BYTES, LDS_BYTES)
    rc, out, msg = plan_spaced(lib, 1024, seeds_with(1024, 16, LDS_FIT + 1))
    assert rc == 1 and out[1] == LDS_BYTES  # BTLBF_EINVAL
    assert "k = 1024" in msg and "16 seeds" in msg and "%d bytes of LDS" % lds_need(1024, LDS_FIT + 1, 1000) in msg and "%d are available" % LDS_BYTES in msg, msg
    # the configuration of the issue: 16 seeds of the lowest weight
    rc, out, msg = plan_spaced(lib, 1024, ["1" + "0" * 1022 + "1"] * 16)
    assert rc == 1 and "%d bytes of LDS" % lds_need(1024, 16 * 1022, 1022) in msg, msg
    # everything the suite has used so far, and smaller k with the most don't-cares, is accepted
    for k, n, z in ((31, 4, 35), (96, 16, 16 * 94), (512, 16, 16 * 510), (900, 16, 16 * 898), (1024, 1, 1022), (1024, 13, 13 * 1022)):
        rc, out, msg = plan_spaced(lib, k, seeds_with(k, n, z))
        distinct = len({i for s in seeds_with(k, n, z) for i, c in enumerate(s) if c == "0"})
        # (a union list of up to 64 entries holds fillers besides the distinct offsets: groups of one mask come in pairs)
        lo, hi = (lds_need(k, z, distinct), lds_need(k, z, 64)) if distinct <= 64 else (lds_need(k, z, distinct),) * 2
        assert rc == 0 and lo <= out[0] <= hi, (k, n, z, out, msg)


@gpu
def test_spaced_lds_largest_configuration_that_fits(bf, oracle):
    """k = 1024, 16 seeds with 14008 don't-care positions in all -- every byte of the 160 KB -- through every family
    that takes such seeds: hash-only, bit filter, 8-bit and wide counters, screen"""
    k, h = 1024, 16
    seeds = seeds_with(k, h, LDS_FIT)
    b = lk.Buf([lk.acgt(np.random.RandomState(3), n).tobytes() for n in (k + 700, k - 1, k + 2049)], "ragged")
    w = lk.Windows(oracle, b, k, h, seeds)
    assert w.idx.size == 701 + 2050
    seq, st = np.frombuffer(b.buf, np.uint8), b.starts
    check_hash_output("hash", bf.sthash_seqs(dev(b.buf, 1), seeds, 1, k, starts=dev_starts(st)), b, w, seeds=True)
    bits = 1 << 20
    body = np.zeros(bits // 8, np.uint8)
    oracle.bf_insert(body, bits, h, w.crows[:701])
    f = bf.BloomFilter(bits, h, k)
    f.setSpacedSeeds(seeds, 1)
    f.insertSeqs(seq[: k + 700])
    assert_same("bit filter body", f.download(), body)
    hit = lk.spread(b.n, w.idx, oracle.bf_contains(body, bits, h, w.crows).astype(bool))
    gh, gv, gc = f.containsSeqs(seq, starts=st, want_counts=True)
    assert_bitmap("contains hit", gh, hit, b.n)
    assert_bitmap("contains valid", gv, w.clean, b.n)
    assert hit.sum() >= 701 and int(gc[1]) == hit.sum()
    out = bf.screenSeqs([f], seq, starts=st)
    import screen_cases as sc

    wseq = mm.window_seqs(b.n, st)
    assert_same("screen hits", sc.host(out[0]).reshape(3, -1)[:, 0].copy(),
                np.bincount(wseq[w.idx], weights=hit[w.idx].astype(np.int64), minlength=3).astype(np.uint32))
    for cbits in (8, 32):
        c = bf.CountingBloomFilter(1 << 16, h, k, 1, counter_bits=cbits)
        c.setSpacedSeeds(seeds, 1)
        c.insertSeqs(seq, starts=st, increment_all=True)
        size = c.size()
        exp = wm.increment_all_exact(np.zeros(size, np.uint64), (w.crows % np.uint64(size)).ravel(), wm.max_of(cbits))
        wm.check_increment_all(c.counters(), exp)
        gm, gv = c.minCountSeqs(seq, starts=st)
        mn = lk.spread(b.n, w.idx, exp[(w.crows % np.uint64(size)).astype(np.int64)].min(axis=1), c.dtype)
        assert_same("u%d min counts" % cbits, np.ascontiguousarray(host(gm)).view(c.dtype), mn)
    # the miBF has limits of its own far below this one (8 hash values per window, 64 distinct don't-care offsets), so
    # its kernels never see such seeds: refused when the miBF is made
    with pytest.raises(bf._lib.BtlbfError) as e:
        bf.MIBloomFilter(f, 2)
    assert e.value.code == bf._lib.EINVAL


@gpu
def test_spaced_lds_smallest_configuration_that_does_not_fit_is_refused(bf):
    """one don't-care position more: BTLBF_EINVAL with the message, from setSpacedSeeds of every filter kind, from
    sthash_seqs and from the miBF's stage-1 filter -- before any kernel is configured or launched (the limit is the
    same for the four direct kernels: one tile size, one bound on their static LDS)"""
    from btl_bloomfilter_amd._lib import EINVAL, BtlbfError

    k, h = 1024, 16
    seeds = seeds_with(k, h, LDS_FIT + 1)
    s = lk.acgt(np.random.RandomState(4), 3000)
    calls = [lambda: bf.BloomFilter(1 << 16, h, k).setSpacedSeeds(seeds, 1),
             lambda: bf.CountingBloomFilter(1 << 16, h, k, 1).setSpacedSeeds(seeds, 1),
             lambda: bf.CountingBloomFilter(1 << 16, h, k, 1, counter_bits=16).setSpacedSeeds(seeds, 1),
             lambda: bf.sthash_seqs(s, seeds, 1, k), lambda: bf.sthash_seqs(dev(s, 0), seeds, 1, k)]
    for i, call in enumerate(calls):
        with pytest.raises(BtlbfError) as e:
            call()
        msg = str(e.value)
        assert e.value.code == EINVAL, (i, msg)
        assert "k = 1024" in msg and "16 seeds" in msg and "%d bytes of LDS" % (LDS_BYTES + 16) in msg and "%d are available" % LDS_BYTES in msg, msg
    # a filter that refused the seeds keeps working with what it had
    f = bf.BloomFilter(1 << 16, h, k)
    good = seeds_with(k, h, 2000)
    f.setSpacedSeeds(good, 1)
    with pytest.raises(BtlbfError):
        f.setSpacedSeeds(seeds, 1)
    f.insertSeqs(s)
    assert f.getPop() > 0
