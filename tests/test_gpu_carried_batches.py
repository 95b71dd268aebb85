"""Carried batches (csrc/part_plan.hpp): a call that does not fit one batch runs K carried batches
-- pass A and one ungrouped pass B each, their segment regions kept as blocks -- and a final batch whose pass C walks its
own regions and the carried ones: one sweep of the array per call.  Everything is compared bit for bit with the direct
kernels, which tests/test_gpu_parity.py pins to the reference's golden vectors and to the CPU oracle
(BloomFilter::insert / contains, BloomFilter.hpp:185-194,252-262; CountingBloomFilter::incrementAll,
CountingBloomFilter.hpp:171-181).

Which plan a call took is read from the profile: pass A runs once per batch (insert_hash / query_hash = K + 1), pass C
once per group of level-0 bins and SWEEP (insert_apply / query_test = 8 under a carried plan, batches x 8 otherwise).

How the plans are forced.  By the planner's own arithmetic a carried block costs what it saves unless the last level is
packed (a 32-bit entry takes 4 bytes in the level-0 buffer and 4 in a block), and on small filters the block's many
short regions cost more than they save at any size below about 10^6 reads.  So:
  * the planner's own choice is tested where it exists: 2^33 bits as 16 bins x 1024 ways (packed), 3 x 10^6 reads, where
    one batch takes 6552 MiB; by part_plan.hpp's arithmetic the planner takes K = 1 from 5904 MiB, K = 2 from 5804 MiB and
    independent batches below that -- the launch counts asserted here are those plans';
  * every other case -- the unpacked 64 x 64 geometry, the short lists of a budget below 2 GiB, the region shapes, the
    counting filter -- takes the carried form through BTLBF_CARRY_FORCE=K, which plans K equal carried batches although
    one batch would fit."""
import pytest

pytestmark = pytest.mark.gpu

L, K, H = 150, 31, 4
W = L - K + 1
MIB = 1 << 20
GROUPS = 8  # 64 level-0 bins in groups of 8; 16 in groups of 2


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    assert m._lib.load().btlbf_device_count() > 0
    return m


def launches(prof, name):
    return prof.get(name, (0, 0))[1]


def assert_plan(prof, kind, batches, sweeps=1):
    """pass A `batches` times, pass C once per group and sweep; kind: "insert" or "query" """
    hash_, apply_ = ("insert_hash", "insert_apply") if kind == "insert" else ("query_hash", "query_test")
    assert launches(prof, hash_) == batches and launches(prof, apply_) == sweeps * GROUPS, (batches, sweeps, prof)


def part_insert(flt, reads, scratch, **kw):
    """the partitioned insert of `reads` under a scratch budget -> the profile of that call"""
    import torch

    flt.setInsertMode("partitioned", scratch_bytes=scratch)
    flt.setProfiling(True)
    flt.getProfile()
    flt.insertSeqs(reads, read_len=L, **kw)
    torch.cuda.synchronize()
    prof = flt.getProfile()
    flt.setProfiling(False)
    assert "insert_direct" not in prof, prof
    return prof


def direct_pair(bf, bits, before=None):
    """two filters holding the reads `before` (direct kernels); a stays on the direct kernels"""
    a, b = bf.BloomFilter(bits, H, K), bf.BloomFilter(bits, H, K)
    for f in (a, b):
        f.setInsertMode("direct")
        if before is not None:
            f.insertSeqs(before, read_len=L)
    return a, b


def check_insert(bf, bits, reads, scratch, batches, fresh, sweeps=1, before=None):
    """fresh: into a cleared filter (the call carries the clear out); else into one that holds `before`"""
    a, b = direct_pair(bf, bits, None if fresh else before)
    if fresh:
        b.insertSeqs(before, read_len=L)
        b.clear()
    a.insertSeqs(reads, read_len=L)
    prof = part_insert(b, reads, scratch)
    assert_plan(prof, "insert", batches, sweeps)
    assert a.digest() == b.digest(), "the partitioned insert differs from the direct kernel"
    assert a.getPop() == b.getPop() > 0
    return a, b


def query_both(a, b, q, scratch):
    """the direct query on a, the partitioned one on b -> (counts, profile of the partitioned call)"""
    import torch

    a.setQueryMode("direct")
    b.setQueryMode("partitioned")
    b.setInsertMode("partitioned", scratch_bytes=scratch)  # the query shares the insert's budget
    ha, va, ca = a.containsSeqs(q, read_len=L, want_counts=True)
    b.setProfiling(True)
    b.getProfile()
    hb, vb, cb = b.containsSeqs(q, read_len=L, want_counts=True)
    torch.cuda.synchronize()
    prof = b.getProfile()
    b.setProfiling(False)
    assert torch.equal(va, vb) and ca.tolist() == cb.tolist(), (ca.tolist(), cb.tolist())
    assert torch.equal(ha, hb), "per-window bitmaps differ"
    return cb.tolist(), prof


# ---- 1: 2^31 bits, 64 bins x 64 ways, 32-bit entries, groups of 8 bins ----------------------------------------------
@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("k_carried", [1, 2, 3])
def test_unpacked_64x64(bf, monkeypatch, k_carried, fresh):
    monkeypatch.setenv("BTLBF_CARRY_FORCE", str(k_carried))
    n = 300_000
    reads, before = bf.synth_reads_device(31, 0, n, L), bf.synth_reads_device(32, 0, 50_000, L)
    check_insert(bf, 1 << 31, reads, 1500 * MIB, k_carried + 1, fresh, before=before)


# ---- 2: 2^33 bits with BTLBF_SPLIT_BITS=10: 16 bins x 1024 ways, packed, groups of 2 --------------------------------
@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("k_carried", [1, 2])
def test_packed_16x1024_short_lists(bf, monkeypatch, k_carried, fresh):
    """a budget below 2 GiB: pass A's plain schedule, the short fail and spill lists"""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    monkeypatch.setenv("BTLBF_CARRY_FORCE", str(k_carried))
    n = 300_000
    reads, before = bf.synth_reads_device(33, 0, n, L), bf.synth_reads_device(34, 0, 50_000, L)
    check_insert(bf, 1 << 33, reads, 2000 * MIB, k_carried + 1, fresh, before=before)


@pytest.fixture(scope="module")
def big_reads(bf):
    return bf.synth_reads_device(35, 0, 3_000_000, L), bf.synth_reads_device(36, 0, 50_000, L)


# the planner's own choice at 3 x 10^6 reads (one batch: 6552 MiB): (budget, carried batches, independent batches)
PLANNED = {"K1": (6200 * MIB, 1, 0), "K2": (5850 * MIB, 2, 0), "none_fits": (4000 * MIB, 0, 2)}


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("plan", ["K1", "K2", "none_fits"])
def test_packed_16x1024_planned(bf, monkeypatch, big_reads, plan, fresh):
    """budgets of 2 GiB and more: pass A's overlapped schedule, the full-size lists; the plan is the planner's.  A budget
    too small for any K: independent batches, a sweep each, the same bits."""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    budget, k_carried, independent = PLANNED[plan]
    reads, before = big_reads
    if k_carried:
        check_insert(bf, 1 << 33, reads, budget, k_carried + 1, fresh, before=before)
    else:
        check_insert(bf, 1 << 33, reads, budget, independent, fresh, sweeps=independent, before=before)


def test_carry_switched_off(bf, monkeypatch, big_reads):
    """BTLBF_CARRY=0 under a budget that holds K = 1: the independent batches of old, identical bits and answers"""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    monkeypatch.setenv("BTLBF_CARRY", "0")
    reads, before = big_reads
    a, b = check_insert(bf, 1 << 33, reads, 6200 * MIB, 2, False, sweeps=2, before=before)
    cnt, prof = query_both(a, b, reads[: 2_000_000 * L], 4000 * MIB)
    assert cnt == [2_000_000 * W] * 2
    assert launches(prof, "query_hash") == 2 and launches(prof, "query_test") == 2 * GROUPS, prof


# ---- 3: carried region shapes ---------------------------------------------------------------------------------------
# 16 bins x 1024 ways, K = 1: the carried block has 16384 segments x 32 writers = 2^19 regions, and the carried batch is
# the first half of the call's tiles (68 reads a tile), 480 entries a read.  640 reads: 5 of 10 tiles carried, 340 reads,
# 0.31 entries per region -- most regions empty, the others one or two entries; 6 600: mean 3.05 -- one partial
# chunk, every length of a last word and a last vector; 105 000: mean 48, sigma 6.9 -- regions one short of a chunk
# (47), on its boundary (48) and a few entries past it, by the thousand each.
@pytest.mark.parametrize("n", [640, 6_600, 105_000])
def test_carried_region_shapes(bf, monkeypatch, n):
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    monkeypatch.setenv("BTLBF_CARRY_FORCE", "1")
    reads = bf.synth_reads_device(37, 0, n, L)
    a, b = check_insert(bf, 1 << 33, reads, 2000 * MIB, 2, True, before=bf.synth_reads_device(38, 0, 100, L))
    q = torch.cat([reads, bf.synth_reads_device(39, 0, max(n // 10, 50), L)])
    (clean, hits), prof = query_both(a, b, q, 2000 * MIB)
    assert_plan(prof, "query", 2)
    assert n * W <= hits < clean


# ---- 4: queries -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def queried(bf, big_reads):
    """two filters of 2^33 bits holding the 3 x 10^6 reads"""
    reads, _ = big_reads
    return direct_pair(bf, 1 << 33, reads)


@pytest.mark.parametrize("plan", ["K1", "K2"])
def test_query_all_hit_and_foreign_reads_in_every_batch(bf, monkeypatch, big_reads, queried, plan):
    """the fail count is zeroed once and one resolve step follows the single test pass: failed positions of the first,
    a middle and the last batch must all clear their windows"""
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    budget, k_carried, _ = PLANNED[plan]
    reads, _ = big_reads
    a, b = queried
    n = 3_000_000
    cnt, prof = query_both(a, b, reads, budget)
    assert_plan(prof, "query", k_carried + 1)
    assert cnt == [n * W, n * W]
    q = reads.clone().view(n, L)
    foreign = bf.synth_reads_device(40, 0, 3_000, L).view(3_000, L)
    for i, at in enumerate((0, n // 2 - 500, n - 1_000)):  # the very first reads, either side of the middle, the last
        q[at: at + 1_000] = foreign[i * 1_000: (i + 1) * 1_000]
    (clean, hits), prof = query_both(a, b, q.reshape(-1), budget)
    assert_plan(prof, "query", k_carried + 1)
    assert launches(prof, "query_resolve") == 1, prof
    assert (n - 3_000) * W <= hits < clean - 2_900 * W


def test_query_miss_heavy_redone_by_the_direct_kernel(bf, monkeypatch, queried):
    """3 x 10^5 foreign reads under a forced K = 2 and a budget below 2 GiB: 1.4 x 10^8 failed probes against a fail list
    of 256 Ki entries -- the whole call is redone by the direct kernel"""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    monkeypatch.setenv("BTLBF_CARRY_FORCE", "2")
    a, b = queried
    q = bf.synth_reads_device(41, 0, 300_000, L)
    (clean, hits), prof = query_both(a, b, q, 2000 * MIB)
    assert_plan(prof, "query", 3)
    assert clean == 300_000 * W and hits < 0.01 * clean


# ---- 5: skew --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies,scratch", [(20_000, 2000 * MIB), (250_000, 2000 * MIB), (30_000, 2100 * MIB)])
def test_skew_spills_of_every_batch_applied_after_the_one_sweep(bf, monkeypatch, copies, scratch):
    """One read repeated in the carried batches and in the final one, as a fresh insert: its 480 positions overrun
    pass A's rings and the carried regions of their segments, and those entries are reported to the spill list, which
    is applied after the single pass C (which would wipe them).  20 000 copies (9.6 x 10^6 probes; the short list of a
    budget below 2 GiB holds 512 Ki): more than the list holds, and the call starts over the ordinary way -- as do 250 000
    copies, which are most of the call.  30 000 copies against the full-size list of 16 Mi entries: it holds them all."""
    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    monkeypatch.setenv("BTLBF_CARRY_FORCE", "2")
    n = 300_000
    reads = bf.synth_reads_device(42, 0, n, L).view(n, L)
    per = copies // 3
    for at in (10_000, 110_000, n - per - 5):  # one run in each of the three batches
        reads[at: at + per] = reads[3].clone()
    reads = reads.reshape(-1)
    a, b = direct_pair(bf, 1 << 33)
    b.insertSeqs(bf.synth_reads_device(43, 0, 1_000, L), read_len=L)
    b.clear()
    a.insertSeqs(reads, read_len=L)
    prof = part_insert(b, reads, scratch)
    # 3 launches of pass A and 8 of pass C -- or twice that where the call started over
    redo = launches(prof, "insert_hash") // 3
    assert redo in (1, 2) and launches(prof, "insert_hash") == 3 * redo and launches(prof, "insert_apply") == GROUPS * redo, prof
    # short list: a run of 6 667 copies is 98 tiles, hashed by 16 workgroups of pass A, so 16 of a hot segment's 32
    # carried regions take 400 entries and more of the read on top of their 90, and hold 288: over 10^6 entries spilled,
    # the list holds 512 Ki.  Full-size list: 1.44 x 10^7 probes of the read at most, the list holds 1.68 x 10^7.
    assert redo == (2 if scratch < 2048 * MIB else 1), prof
    assert a.digest() == b.digest() and a.getPop() == b.getPop() > 0


# ---- 6: counting filter ---------------------------------------------------------------------------------------------
def test_counting_filter_increment_all_twice(bf, monkeypatch):
    """2^28 counters: 4096 segments as 64 x 64, 32-bit entries with exact counts.  incrementAll of the same reads twice
    under a forced K = 2, 200 copies of one read among them: its counters pass 255 in the second call and stay there,
    every other counter holds exactly twice its number of probes -- no entry applied twice, none dropped."""
    import torch

    monkeypatch.setenv("BTLBF_CARRY_FORCE", "2")
    n = 200_000
    reads = bf.synth_reads_device(44, 0, n, L).view(n, L)
    for at in (1_000, 100_000, n - 300):
        reads[at: at + 67] = reads[5].clone()
    reads = reads.reshape(-1)
    a, b = bf.CountingBloomFilter(1 << 28, H, K, 2), bf.CountingBloomFilter(1 << 28, H, K, 2)
    a.setInsertMode("direct")
    for _ in range(2):
        a.insertSeqs(reads, read_len=L, increment_all=True)
        prof = part_insert(b, reads, 1500 * MIB, increment_all=True)
        assert_plan(prof, "insert", 3)
        assert a.digest() == b.digest(), "counters differ from the direct kernel's"
    body = torch.from_numpy(b.download())
    assert int((body == 255).sum()) >= 100 and int(body.max()) == 255  # the repeated read's counters are saturated
