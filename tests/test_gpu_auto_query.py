"""contains() over fixed-length reads in AUTO mode -- the sampled decision (decide_route, host_query.cpp) and its two
split routes -- where it decides: buffers of 2^20 reads and more (the two-stage sampler), counting filters, and the
input shapes the split path is not given elsewhere.

Every case is held against two references at once:

* the whole buffer against the direct kernel of the same filter (setQueryMode("direct")): hit bitmap, valid bitmap and
  counts, word for word, for the AUTO call with the valid bitmap, without it, and with no bitmap at all;
* slices of whole reads against the CPU oracle, from the filter body downloaded once (auto_query_slices.py): both ends
  of the buffer and either side of a 1024-word chunk boundary of the flag array, bit for bit; the windows that would
  straddle two reads must be 0 in both bitmaps.

Which path ran is read from the profile (setProfiling / getProfile).  The spans a call records:

  query_hash     one per batch of the partitioned pipeline (pass A)
  query_test     one per group of level-0 bins and batch (the test pass)
  query_direct   the gather kernel: over the whole buffer of a bit filter (a counting filter's whole-buffer call is
                 recorded as "other"), or over the compacted cold reads of a split call -- one launch either way
  query_resolve  one per sampler launch, one per partitioned batch (fail set + resolve) and, in a split call, one for
                 the prefix sums + gather / compaction and one for the merge of the bitmaps

so that  partitioned whole buffer = hash and no direct / other,  gather kernel only = direct (other) and no hash,
split = both, and the sampler launches are  resolve - hash  (partitioned),  resolve  (gather),  resolve - hash - 2
(split): 1 below 2^20 reads, and from 2^20 reads on 1 when the first look (one read in 64) decided, 2 when the look at
every read did.  The two split executors -- "split_cold": the cold reads gathered and the partitioned query run over the
whole buffer under a read mask, when 4 * n_cold <= n_reads; "split_warm": warm and cold reads both compacted, otherwise
-- record the same spans in a call that asks for a bitmap; in a call that asks for counts only the warm + cold executor
has no bitmaps to merge and records one query_resolve fewer, which is how the tests tell the two apart.

The sampler only steers speed -- every path computes the exact contains() --, so a sampler that reads the wrong bytes or
compares with the wrong threshold shows in the path assertions, a wrong prefix sum or merge in the bitmaps."""
import ctypes as C

import numpy as np
import pytest

from auto_query_slices import bitmap_bits, clean_windows, expected_slice_bits, slice_ranges

pytestmark = pytest.mark.gpu

CAP = 1 << 30  # a scratch budget below 2 GiB: the partitioned query then has a fail list of 256 Ki entries (part_tail)


@pytest.fixture(scope="module")
def bf():
    # torch first, as in every production flow: its HIP runtime and context are up before the library's first call
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    assert m._lib.load().btlbf_device_count() > 0, "GPU tests need a GPU (and the HIP library)"
    return m


def _np(x):
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def _counts_only(flt, q, L):
    """contains() with neither bitmap asked for (what the C++ shim's countReads calls) -> [clean windows, hits]"""
    from btl_bloomfilter_amd import engine as e

    b = e._Buf(q)
    lay, _ = e._layout(None, L, b.mem)
    cnt, p_cnt = e._out(b, 2, np.uint64)
    e.check(flt._L.btlbf_contains_seqs(flt._h, b.ptr, b.nbytes, C.byref(lay), None, None, p_cnt, b.mem,
                                       e._stream_ptr(None, b.keep)))
    return _np(cnt).tolist()


def _assert_path(prof, path, looks, counting, merges=True):
    c = {name: v[1] for name, v in prof.items()}
    n_hash, n_test, n_res = c.get("query_hash", 0), c.get("query_test", 0), c.get("query_resolve", 0)
    n_direct, n_other = c.get("query_direct", 0), c.get("other", 0)
    if path == "partitioned":
        assert n_hash >= 1 and n_test >= n_hash and n_direct == 0 and n_other == 0, prof
        seen = n_res - n_hash
    elif path == "gather":
        assert n_hash == 0 and n_test == 0, prof
        assert (n_direct, n_other) == ((0, 1) if counting else (1, 0)), prof
        seen = n_res
    else:
        assert path in ("split_cold", "split_warm")
        assert n_hash >= 1 and n_test >= n_hash and n_direct == 1 and n_other == 0, prof
        seen = n_res - n_hash - (2 if merges else 1)
    assert seen == looks, ("sampler launches", seen, looks, prof)


def check_auto(flt, oracle, body, params, q, L, path, looks, large=False):
    """AUTO against the direct kernel (whole buffer, three call shapes) and against the oracle (slices); the path each
    AUTO call took.  q: device tensor or numpy array.  Returns the counts."""
    import torch

    k = params["k"]
    n_bytes = q.numel() if hasattr(q, "numel") else q.size
    n_reads = n_bytes // L
    assert n_reads * L == n_bytes
    counting = params["kind"] == "cbf"
    flt.setQueryMode("direct")
    hit_d, valid_d, cnt_d = (_np(x) for x in flt.containsSeqs(q, read_len=L, want_valid=True, want_counts=True))
    cnt_d = cnt_d.tolist()
    flt.setQueryMode("auto")
    flt.setProfiling(True)
    profs = []
    try:
        flt.getProfile()
        hit_a, valid_a, cnt_a = (_np(x) for x in flt.containsSeqs(q, read_len=L, want_valid=True, want_counts=True))
        torch.cuda.synchronize()
        profs.append(flt.getProfile())
        hit_b, none_b, cnt_b = flt.containsSeqs(q, read_len=L, want_valid=False, want_counts=True)
        torch.cuda.synchronize()
        profs.append(flt.getProfile())
        cnt_c = _counts_only(flt, q, L)
        torch.cuda.synchronize()
        profs.append(flt.getProfile())
    finally:
        flt.setProfiling(False)
    print("%s/%d expected:" % (path, looks), [{name: v[1] for name, v in p.items()} for p in profs], cnt_d)
    # 1. the whole buffer, word for word
    assert cnt_a.tolist() == cnt_d and _np(cnt_b).tolist() == cnt_d and cnt_c == cnt_d
    assert none_b is None
    assert (hit_a == hit_d).all() and (valid_a == valid_d).all() and (_np(hit_b) == hit_d).all()
    # 2. the counts against the buffer itself, the slices against the oracle
    host = _np(q)
    assert cnt_d[0] == clean_windows(host, L, k)
    assert cnt_d[1] <= cnt_d[0]
    for r0, r1 in slice_ranges(n_reads, large):
        eh, ev = expected_slice_bits(oracle, body, params, host[r0 * L: r1 * L], L)
        assert (bitmap_bits(valid_a, r0 * L, r1 * L) == ev).all(), ("valid", r0, r1)
        assert (bitmap_bits(hit_a, r0 * L, r1 * L) == eh).all(), ("hit", r0, r1)
    # 3. the path each of the three AUTO calls took (last: a failure here says that the answers above were right)
    for prof in profs[:2]:
        _assert_path(prof, path, looks, counting)
    _assert_path(profs[2], path, looks, counting, merges=path != "split_warm")  # (counts only: nothing to merge)
    return cnt_d


def splice(bf, q, n, L, idx, seed=43):
    """reads `idx` (numpy) of the device buffer q replaced by foreign reads (another seed of the generator)"""
    import torch

    if len(idx):
        t = torch.from_numpy(np.asarray(idx, np.int64)).cuda()
        q.view(n, L)[t] = bf.synth_reads_device(seed, 0, len(idx), L).view(len(idx), L)
    return q


# ---------------------------------------------------------------------------------------------
# case 1: the two-stage sampler, bit filter
# ---------------------------------------------------------------------------------------------
K1, H1, L1, N1 = 31, 4, 60, (1 << 20) + 77  # W = 30; 63 MB; n is a multiple of neither 64 nor 256


@pytest.fixture(scope="module")
def case1(bf):
    """get(bits) -> (filter with the N1 reads of seed 42 inserted, its body, oracle parameters); the reads"""
    reads = bf.synth_reads_device(42, 0, N1, L1)
    made = {}

    def get(bits):
        if bits not in made:
            flt = bf.BloomFilter(bits, H1, K1)
            flt.setInsertMode("auto", scratch_bytes=CAP)
            flt.insertSeqs(reads, read_len=L1)
            made[bits] = (flt, flt.download(), {"kind": "bf", "bits": bits, "h": H1, "k": K1})
        return made[bits]

    return get, reads


SPECIAL = [0, 63, 64, 65535, 65536, 65537, 15 * 65536, N1 - 1]  # ends of flag words and of 1024-word flag chunks


def _case1_foreign(sub):
    rng = np.random.default_rng(20)
    if sub == "a":
        return np.zeros(0, np.int64)
    if sub == "b":
        return np.arange(N1)
    if sub in ("c", "c_short", "g"):
        return np.union1d(np.flatnonzero(rng.random(N1) < 0.001), SPECIAL)
    if sub == "d":
        return np.flatnonzero(rng.random(N1) < 0.01)
    if sub == "e":
        return np.arange(0, N1, 10)
    assert sub == "f"
    return np.flatnonzero(rng.random(N1) < 0.4)


@pytest.mark.parametrize("sub,bits,path,looks", [
    ("a", 1 << 30, "partitioned", 1), ("b", 1 << 30, "gather", 1), ("c", 1 << 30, "split_cold", 2),
    ("c_short", 1 << 30, "split_cold", 2), ("d", 1 << 30, "split_cold", 2), ("d", 3 << 28, "split_cold", 2),
    ("e", 1 << 30, "split_cold", 2), ("f", 1 << 30, "split_warm", 2), ("g", 1 << 30, "partitioned", 2)])
def test_two_stage_sampler_bit_filter(bf, oracle, case1, sub, bits, path, looks):
    """N1 = 2^20 + 77 reads of 60 bytes, k = 31 (W = 30), h = 4, in a filter of 2^30 (or 3 x 2^28: the sampler's
    non-power-of-two modulo) bits, about 11 % (14 %) full after the N1 inserts: a foreign window is a false positive
    with probability 1.5e-4 (4.4e-4), so foreign reads are sampled cold and inserted reads warm.

    From 2^20 reads on decide_route first looks at one read in 64 -- n_s = 16386 reads -- and derives cold_frac and
    the second sample's probes from it.  With the 1 GiB scratch cap the fail list has 256 Ki entries and few_cold =
    0.25 * 262144 / (W * h) = 546 reads; with the default budget 4 Mi entries and few_cold = 8738.

    a  no foreign read: none cold among 16386, and n * 8 / n_s = 512 < 546 -> partitioned after the first look
    b  all foreign: no warm read in the sample -> gather kernel after the first look
    c  0.1 % foreign at seeded positions plus the reads at the ends of flag words and flag chunks (SPECIAL): the first
       look sees 16.4 +- 4.0 cold reads, the band for probes2 = (h + 1) / 2 = 2 ends at 0.0025 * 16386 = 41 (6 sigma);
       n_cold ~ 1057 >= 546 -> split; 4 * n_cold <= n: the cold-only executor (gather under a read mask)
    c_short  c without its last three reads: the bitmaps end inside a word
    d  1 %: 164 +- 12.7 cold reads at the first look, inside (41, 410] by 9 sigma -> probes2 = 3; cold-only executor
    e  every 10th read (a period the first look's pseudo-random offsets must not lock onto): cold_frac 0.1 ->
       probes2 = h; cold-only executor (4 * n / 10 <= n)
    f  40 %: the warm + cold executor (both compacted, bitmaps merged)
    g  c with the default scratch budget: n_cold ~ 1057 < 8738 -> the whole buffer partitioned after the second look,
       the foreign reads' failures through the fail list

    One warm and one cold read carry an N at byte 7.  (With k = 31 > W every byte of a read lies in a sampled window;
    byte 7 makes only the sample at offset 0 unclean, and the other two still vote.)"""
    get, reads = case1
    flt, body, params = get(bits)
    idx = _case1_foreign(sub)
    q = splice(bf, reads.clone(), N1, L1, idx)
    is_foreign = np.zeros(N1, bool)
    is_foreign[idx] = True
    n_with_n = 0
    if not is_foreign.all():
        q[int(np.flatnonzero(~is_foreign)[101]) * L1 + 7] = ord("N")
        n_with_n += 1
    if is_foreign.any():
        q[int(idx[idx >= 60][0]) * L1 + 7] = ord("N")
        n_with_n += 1
    n = N1
    if sub == "c_short":
        n = N1 - 3
        q = q[: n * L1]
        assert (n * L1) % 64 and is_foreign[N1 - 1]
    flt.setInsertMode("auto", scratch_bytes=0 if sub == "g" else CAP)
    try:
        cnt = check_auto(flt, oracle, body, params, q, L1, path, looks, large=True)
    finally:
        flt.setInsertMode("auto", scratch_bytes=CAP)
    W = L1 - K1 + 1
    assert cnt[0] == n * W - 8 * n_with_n  # an N at byte 7 takes the windows at offsets 0 .. 7
    if sub == "a":
        assert cnt[1] == cnt[0]
    elif sub == "b":
        assert cnt[1] <= 0.001 * cnt[0]  # from the fill ratio: 1.5e-4 expected
    else:
        assert cnt[1] >= (n - len(idx)) * W - 8


# ---------------------------------------------------------------------------------------------
# case 2: a counting filter through AUTO
# ---------------------------------------------------------------------------------------------
K2, H2, L2, N2 = 25, 3, 150, 40000


@pytest.fixture(scope="module")
def case2(bf):
    """reads 0 .. 19999 inserted twice (three of them 302 times), reads 20000 .. 39999 once, in a filter with
    threshold 2 and one with threshold 1 (the same counters)"""
    import torch

    reads = bf.synth_reads_device(21, 0, N2, L2)
    flt = bf.CountingBloomFilter(1 << 27, H2, K2, 2)
    flt.insertSeqs(reads, read_len=L2, increment_all=True)
    flt.insertSeqs(reads[: 20000 * L2], read_len=L2, increment_all=True)
    flt.insertSeqs(reads[: 3 * L2].repeat(300), read_len=L2, increment_all=True)
    torch.cuda.synchronize()
    body = flt.download()
    assert body.max() == 255
    one = bf.CountingBloomFilter(1 << 27, H2, K2, 1)
    one.upload(body)
    return reads, body, {2: flt, 1: one}


def _interleave(period):
    """read i of the query: every period-th one (i % period == period - 1) inserted once, the others twice"""
    i = np.arange(N2)
    once = i % period == period - 1
    return np.where(once, 20000 + (i // period) % 20000, (i - i // period) % 20000)


@pytest.mark.parametrize("what,thr,path", [("twice", 2, "partitioned"), ("twice_one_vote", 2, "partitioned"),
                                           ("once", 2, "gather"), ("9to1", 2, "split_cold"), ("1to1", 2, "split_warm"),
                                           ("9to1", 1, "partitioned")])
def test_counting_filter_through_auto(bf, oracle, case2, what, thr, path):
    """CountingBloomFilter(2^27, h = 3, k = 25), L = 150 (W = 126): the sampler compares counters with the threshold,
    the cold-only executor runs the counting partitioned query under a read mask, the hits are recounted from the
    merged bitmap.  The filter holds 2.3e7 increments in 1.3e8 counters: a counter of a read inserted once stands at
    2 or more with probability 0.16, a window of such a read passes threshold 2 with 0.4 %, so those reads are cold at
    threshold 2 and warm at threshold 1.  Fewer than 2^20 reads: one sampler launch.  Every query passes worth_sweep
    (>= 20000 * 126 * 3 = 7.6e6 probes), and few_cold (default budget) is 0.25 * 2^22 / 378 = 2774 reads.

    twice  reads 0 .. 19999: every counter >= 2 -> partitioned
    twice_one_vote  the same reads with two of the three samples (offsets 0, 63, 125) made unclean by an N, a different
           pair in every third read: each of the sampler's three comparisons with the threshold then decides a third
           of the reads alone (in `twice` the majority of three hides one wrong comparison), and a counter that stands
           at exactly the threshold must count as a hit -> still partitioned
    once  reads 20000 .. 39999: nothing warm -> gather kernel
    9to1   40000 reads, every 10th inserted once: 4000 cold >= 2774 -> split, the cold-only executor
    1to1   every other read inserted once: 20000 cold, 20000 warm (7.6e6 probes) -> split, warm + cold
    9to1 at threshold 1: the same buffer, the same counters, every read warm -> partitioned"""
    import torch

    reads, body, flts = case2
    flt = flts[thr]
    if what == "twice":
        q = reads[: 20000 * L2]
    elif what == "twice_one_vote":
        q = reads[: 20000 * L2].clone()
        rows = q.view(20000, L2)
        # an N at byte 0 / 75 / 149 takes the sample at offset 0 / 63 / 125 (and no other sample) out of the vote
        for vote, kill in enumerate(((75, 149), (0, 149), (0, 75))):
            for b in kill:
                rows[vote::3, b] = ord("N")
    elif what == "once":
        q = reads[20000 * L2:]
    else:
        src = _interleave(10 if what == "9to1" else 2)
        q = reads.view(N2, L2)[torch.from_numpy(src).cuda()].reshape(-1).contiguous()
    params = {"kind": "cbf", "h": H2, "k": K2, "thr": thr}
    cnt = check_auto(flt, oracle, body, params, q, L2, path, 1)
    W = L2 - K2 + 1
    n = q.numel() // L2
    assert cnt[0] == n * W or (what == "twice_one_vote" and n * (W - 2 * K2) < cnt[0] < n * W)
    if what.startswith("twice") or thr == 1:
        assert cnt[1] == cnt[0]
    elif what == "once":
        assert 0 < cnt[1] < 0.05 * cnt[0]
    else:
        warm = n - n // (10 if what == "9to1" else 2)
        assert warm * W <= cnt[1] < warm * W + 0.05 * (n - warm) * W


# ---------------------------------------------------------------------------------------------
# case 3: sampler edges (bit filter of 2^30 bits, h = 4, about a third of the reads foreign)
# ---------------------------------------------------------------------------------------------
BITS3, H3 = 1 << 30, 4


def _third_foreign(bf, reads, n, L):
    return splice(bf, reads.clone(), n, L, np.arange(n // 3) * 3 + 1)


def _filter3(bf, reads, L, k, cap=0):
    flt = bf.BloomFilter(BITS3, H3, k)
    if cap:
        flt.setInsertMode("auto", scratch_bytes=cap)
    flt.insertSeqs(reads, read_len=L)
    return flt, flt.download(), {"kind": "bf", "bits": BITS3, "h": H3, "k": k}


@pytest.mark.parametrize("mis", [1, 5, 15])
@pytest.mark.parametrize("L,n", [(150, 40000), (151, 40000), (37, 300000)])
def test_split_query_misaligned_device_pointers(bf, oracle, L, n, mis):
    """read_sample_kernel<STAGED> copies its 256 reads from the 16-byte boundary below them and takes the windows
    back out at `mis` bytes from it: AUTO on a buffer that starts 1, 5 or 15 bytes past a 16-byte boundary.  A third
    of the reads foreign: split, the warm + cold executor (L = 37, k = 31: W = 7, where a sampler that is a few bytes
    off straddles two reads with every sample, calls every read cold and sends the buffer to the gather kernel)."""
    import torch

    k = 31
    reads = bf.synth_reads_device(42, 0, n, L)
    flt, body, params = _filter3(bf, reads, L, k)
    t = torch.zeros(n * L + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    q = t[mis: mis + n * L]
    q.copy_(_third_foreign(bf, reads, n, L))
    q[5 * L + 3] = ord("N")
    assert q.data_ptr() % 16 == mis
    check_auto(flt, oracle, body, params, q, L, "split_warm", 1)


@pytest.mark.parametrize("L,foreign,cap,path", [(32, "third", 0, "gather"), (32, "3%", CAP, "split_cold"), (33, "third", 0, "split_warm")])
def test_two_stage_sampler_one_and_two_windows_per_read(bf, oracle, L, foreign, cap, path):
    """k = 32 with L = 32 (W = 1: one sample per read) and L = 33 (W = 2: two samples), n = 2^20 + 197 reads, so both
    looks of the sampler run.

    W = 2, a third foreign: few_cold = 0.25 * 2^22 / 8 = 131072 < n / 3, the warm reads have 5.6e6 probes -> split, the
    warm + cold executor.
    W = 1: the buffer has 4.195e6 probes, just over worth_sweep's floor of 4e6 (and over 0.0165 * 2^27 bytes = 2.2e6).
    With a third foreign the first look lets it pass -- (n_s - n_cold) * 64 * 1.5 * 4 = 4.195e6 +- 2.3e4 --, the look at
    every read then finds 2.8e6 warm probes, not worth a sweep: the gather kernel, after two looks.  The split path
    needs warm * 4 >= 4e6, that is at most 48773 cold reads, and more than few_cold: 16384 with the 1 GiB scratch cap
    (262144 without it, so only with it).  30000 foreign reads (2.9 %: cold_frac > 0.025, probes2 = h) -> split, the
    cold-only executor."""
    k, n = 32, (1 << 20) + 64 * 3 + 5
    reads = bf.synth_reads_device(42, 0, n, L)
    flt, body, params = _filter3(bf, reads, L, k, cap)
    if foreign == "third":
        q = _third_foreign(bf, reads, n, L)
    else:
        q = splice(bf, reads.clone(), n, L, np.sort(np.random.default_rng(3).choice(n, 30000, replace=False)))
    q[7 * L + 3] = ord("N")
    cnt = check_auto(flt, oracle, body, params, q, L, path, 2, large=True)
    assert cnt[0] == (n - 1) * (L - k + 1)


def test_split_query_reads_without_a_clean_sample(bf, oracle):
    """L = 100, k = 31 (W = 70: samples at offsets 0, 35 and 69), 60000 reads, a third foreign, and whole reads
    overwritten: 500 all N (no clean window), 500 with an N exactly at bytes 0, 35 and 69 (every sample unclean, clean
    windows in between: nothing to vote with, the read goes warm), 500 inserted reads in lower case, 500 inserted reads
    with one N at byte 50 (only the middle sample unclean).  Split, the warm + cold executor."""
    import torch

    L, k, n = 100, 31, 60000
    W = L - k + 1
    reads = bf.synth_reads_device(42, 0, n, L)
    flt, body, params = _filter3(bf, reads, L, k)
    q = _third_foreign(bf, reads, n, L)
    fixed = np.array([0, 63, 64, n - 1])  # ends of the buffer and of a flag word
    perm = np.random.default_rng(8).permutation(np.setdiff1d(np.arange(n), fixed))
    anywhere = np.concatenate([fixed, perm[:996]])  # warm and foreign reads alike
    inserted = perm[996:][perm[996:] % 3 != 1][:1000]
    rows = q.view(n, L)

    def dev(a):
        return torch.from_numpy(np.asarray(a, np.int64)).cuda()

    rows[dev(anywhere[:500])] = ord("N")
    for b in (0, W // 2, W - 1):
        rows[dev(anywhere[500:]), b] = ord("N")
    low = dev(inserted[:500])
    rows[low] = rows[low] | 0x20
    rows[dev(inserted[500:]), 50] = ord("N")
    assert len(inserted) == 1000 and len(np.unique(np.concatenate([anywhere, inserted]))) == 2000
    check_auto(flt, oracle, body, params, q, L, "split_warm", 1)


def test_split_query_host_memory(bf, oracle):
    """the L = 150 buffer from host memory into host outputs: staged, answered by the split path, copied back"""
    L, k, n = 150, 31, 40000
    reads = bf.synth_reads_device(42, 0, n, L)
    flt, body, params = _filter3(bf, reads, L, k)
    q = _third_foreign(bf, reads, n, L)
    q[5 * L + 3] = ord("N")
    check_auto(flt, oracle, body, params, q.cpu().numpy(), L, "split_warm", 1)


def test_split_query_scratch_regrowth(bf, oracle):
    """the flag array and the compacted buffers are cached in the filter and regrown: half the buffer, then all of
    it, then the opposite cold ratio (two thirds foreign), then a cold-only call, on one filter"""
    L, k, n = 150, 31, 40000
    reads = bf.synth_reads_device(42, 0, n, L)
    flt, body, params = _filter3(bf, reads, L, k)
    q = _third_foreign(bf, reads, n, L)
    check_auto(flt, oracle, body, params, q[: (n // 2) * L], L, "split_warm", 1)
    check_auto(flt, oracle, body, params, q, L, "split_warm", 1)
    idx = np.flatnonzero(np.arange(n) % 3 != 1)
    check_auto(flt, oracle, body, params, splice(bf, reads.clone(), n, L, idx, seed=44), L, "split_warm", 1)
    # 10 % cold (4000 >= few_cold = 0.25 * 2^22 / 480 = 2184): the cold-only executor over the same cached buffers
    check_auto(flt, oracle, body, params, splice(bf, reads.clone(), n, L, np.arange(0, n, 10)), L, "split_cold", 1)
    check_auto(flt, oracle, body, params, q[: (n // 2) * L], L, "split_warm", 1)
