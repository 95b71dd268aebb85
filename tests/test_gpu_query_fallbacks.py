"""contains() and insert when the route that was chosen cannot run: the partition scratch does not fit its budget, so
the partitioned pipeline declines (part_prepare not ok) and every route that builds on it downgrades (host_query.cpp).

The budget is setInsertMode(mode, scratch_bytes=1 << 20): the tail of the scratch alone -- fail list and failed-position
table -- is about 6.3 MiB for budgets below 2 GiB (part_tail), so no plan fits, not even one of a single tile.  The
filter is the shape of test_split_query_scratch_regrowth (2^30 bits, h = 4, k = 31, L = 150, 40000 reads) and is filled
before the budget is set.

Every query is held against setQueryMode("direct") of the same filter as check_auto (test_gpu_auto_query.py) does: hit
bitmap, valid bitmap and counts, word for word, for the call with the valid bitmap, without it, and with no bitmap at
all.  Which way the call went is read from the profile; the spans are those test_gpu_auto_query.py describes:

  forced partitioned   the partitioned query declines before its first launch; the direct kernel runs over the whole
                       buffer: query_direct 1, nothing else
  AUTO, SplitCold      one sampler launch, then prefix sums + gather of the cold reads (issued before the masked
                       partitioned query declines, and they stay issued): query_resolve 2; the direct kernel over the
                       whole buffer: query_direct 1
  AUTO, SplitWarm      one sampler launch, prefix sums + compaction, the gather kernel over the warm AND over the cold
                       buffer (query_direct 2), the merge of the bitmaps where one was asked for: query_resolve 3, and
                       2 in the counts-only call

and no query_hash / query_split / query_test / other in any of them."""
import numpy as np
import pytest

from test_gpu_auto_query import _counts_only, _np, bf, splice  # noqa: F401  (bf: fixture)

pytestmark = pytest.mark.gpu

BITS, H, K, L, N = 1 << 30, 4, 31, 150, 40000
TINY = 1 << 20  # scratch budget in bytes


@pytest.fixture(scope="module")
def filled(bf):
    """the filter with the N reads of seed 42 inserted, then given the budget no plan fits; the reads"""
    reads = bf.synth_reads_device(42, 0, N, L)
    flt = bf.BloomFilter(BITS, H, K)
    flt.insertSeqs(reads, read_len=L)
    flt.setInsertMode("auto", scratch_bytes=TINY)
    return flt, reads


def _query_spans(prof):
    return {name: v[1] for name, v in prof.items() if name.startswith("query_") or name == "other"}


def check_fallback(flt, q, mode, direct, resolve, resolve_counts_only):
    """`mode` against the direct kernel (whole buffer, three call shapes); the spans of each of the three calls"""
    import torch

    flt.setQueryMode("direct")
    hit_d, valid_d, cnt_d = (_np(x) for x in flt.containsSeqs(q, read_len=L, want_valid=True, want_counts=True))
    cnt_d = cnt_d.tolist()
    flt.setQueryMode(mode)
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
        flt.setQueryMode("auto")
    spans = [_query_spans(p) for p in profs]
    print(mode, "spans:", spans, cnt_d)
    assert cnt_a.tolist() == cnt_d and _np(cnt_b).tolist() == cnt_d and cnt_c == cnt_d
    assert none_b is None
    assert (hit_a == hit_d).all() and (valid_a == valid_d).all() and (_np(hit_b) == hit_d).all()
    assert cnt_d[0] == (q.numel() // L) * (L - K + 1) and 0 < cnt_d[1] <= cnt_d[0]

    def want(n_resolve):
        return {name: n for name, n in (("query_direct", direct), ("query_resolve", n_resolve)) if n}

    assert spans == [want(resolve), want(resolve), want(resolve_counts_only)], spans
    return cnt_d


def test_forced_partitioned_query_without_scratch(filled):
    """a) setQueryMode("partitioned"), every read present: Partitioned, downgraded to the direct kernel"""
    flt, reads = filled
    cnt = check_fallback(flt, reads, "partitioned", direct=1, resolve=0, resolve_counts_only=0)
    assert cnt[1] == cnt[0]


def test_split_cold_without_scratch(bf, filled):
    """b) AUTO, every 10th read foreign: 4000 cold reads >= few_cold = 0.25 * 2^18 / 480 = 137 (the short fail list of a
    budget below 2 GiB), the 36000 warm reads are worth a sweep, 4 * n_cold <= n: SplitCold, whose masked partitioned
    query declines -- the direct kernel answers the whole buffer"""
    flt, reads = filled
    q = splice(bf, reads.clone(), N, L, np.arange(0, N, 10))
    cnt = check_fallback(flt, q, "auto", direct=1, resolve=2, resolve_counts_only=2)
    assert cnt[1] >= (N - N // 10) * (L - K + 1)


def test_split_warm_without_scratch(bf, filled):
    """c) AUTO, a third of the reads foreign: SplitWarm, whose warm partitioned query declines -- the gather kernel
    answers the warm buffer as well as the cold one, and the call is still answered by the split path"""
    flt, reads = filled
    q = splice(bf, reads.clone(), N, L, np.arange(N // 3) * 3 + 1)
    cnt = check_fallback(flt, q, "auto", direct=2, resolve=3, resolve_counts_only=2)
    assert cnt[1] >= (N - N // 3) * (L - K + 1)


def test_forced_partitioned_insert_without_scratch(bf, filled):
    """d) setInsertMode("partitioned") with the same budget on an empty filter: the partitioned insert declines, the
    direct kernel inserts -- one insert_direct span, no pass A, and the array of a filter filled in direct mode"""
    import torch

    _, reads = filled
    direct = bf.BloomFilter(BITS, H, K)
    direct.setInsertMode("direct")
    direct.insertSeqs(reads, read_len=L)
    flt = bf.BloomFilter(BITS, H, K)
    flt.setInsertMode("partitioned", scratch_bytes=TINY)
    flt.setProfiling(True)
    try:
        flt.getProfile()
        flt.insertSeqs(reads, read_len=L)
        torch.cuda.synchronize()
        prof = flt.getProfile()
    finally:
        flt.setProfiling(False)
    spans = {name: v[1] for name, v in prof.items()}
    print("insert spans:", spans)
    assert spans.get("insert_direct", 0) == 1 and spans.get("insert_hash", 0) == 0, spans
    assert spans == {"insert_direct": 1}, spans
    assert flt.digest() == direct.digest()
    assert flt.digest() != bf.BloomFilter(BITS, H, K).digest()  # (and it is not the digest of an empty array)
