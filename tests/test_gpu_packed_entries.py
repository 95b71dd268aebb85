"""Packed entries between passes B and C: the last split level writes its chunks with three 20-bit entries per 64-bit
word (48 per 128-byte line, csrc/internal.hpp kPackChunk) when it splits 513..1024 ways into segments of at most 2^20
positions (host_partition.cpp plan_caps).  BTLBF_SPLIT_BITS=10 forces such a 1024-way last split on small filters;
everything is compared with the direct kernels, which tests/test_gpu_parity.py pins to the reference's golden vectors
and to the CPU oracle: BloomFilter::insert / contains (BloomFilter.hpp:185-194,252-262).

Counting filters keep 32-bit entries on every level, so there is no counting case here (tests/test_gpu_big.py covers the
1024-way split of a counting filter)."""
import pytest
from conftest import require_hbm

pytestmark = pytest.mark.gpu

L, K, H = 150, 31, 4


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    assert m._lib.load().btlbf_device_count() > 0
    return m


def insert_both(bf, bits, reads, scratch=None):
    """the same reads through the direct kernels (a) and the partitioned pipeline (b): identical arrays"""
    import torch

    a, b = bf.BloomFilter(bits, H, K), bf.BloomFilter(bits, H, K)
    a.setInsertMode("direct")
    if scratch:
        b.setInsertMode("partitioned", scratch_bytes=scratch)
    else:
        b.setInsertMode("partitioned")
    b.setProfiling(True)
    a.insertSeqs(reads, read_len=L)
    b.insertSeqs(reads, read_len=L)
    torch.cuda.synchronize()
    prof = b.getProfile()
    assert prof["insert_split"][1] >= 1 and prof["insert_apply"][1] >= 1 and "insert_direct" not in prof, prof
    assert a.digest() == b.digest(), "partitioned insert through packed entries differs from the direct kernel"
    assert a.getPop() == b.getPop() > 0
    return a, b


def query_both(a, b, q):
    """the same query through the direct kernel on a and the partitioned pipeline on b: identical bitmaps and counts"""
    import torch

    a.setQueryMode("direct")
    b.setQueryMode("partitioned")
    ha, va, ca = a.containsSeqs(q, read_len=L, want_counts=True)
    hb, vb, cb = b.containsSeqs(q, read_len=L, want_counts=True)
    assert torch.equal(va, vb) and ca.tolist() == cb.tolist()
    assert torch.equal(ha, hb), "per-window bitmaps differ"
    return cb.tolist()


def test_bit_filter_2p31_19_bit_entries(bf, monkeypatch):
    """4096 segments of 64 KiB as 4 bins x 1024 ways: 19-bit entries, packed.  Insert, all-hit query, and a query of
    foreign reads, whose clear bits come back through the fail list from packed entries."""
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    n = 300_000
    reads = bf.synth_reads_device(21, 0, n, L)
    a, b = insert_both(bf, 1 << 31, reads)
    b.setQueryMode("partitioned")
    _, _, cnt = b.containsSeqs(reads, read_len=L, want_valid=False, want_counts=True)
    assert cnt.tolist() == [n * (L - K + 1), n * (L - K + 1)]
    foreign = bf.synth_reads_device(22, 0, 20_000, L)
    clean, hits = query_both(a, b, torch.cat([reads[: 5_000 * L], foreign, reads[7_000 * L: 9_000 * L]]))
    assert 7_000 * 120 <= hits < clean - 19_000 * 120


# 4 bins x 1024 ways: 4096 segments x 128 slices (split_slices on 256 CUs) = 2^19 regions, and n reads are 480 n entries
# spread evenly over them.
# 300 reads: 0.27 entries per region -- most (segment, region) pairs are empty, the others hold one or two entries;
# 3 300: mean 3.0 -- regions of 1, 2, 3, 5, 6 entries and more, a single partial chunk each (the last word and the last
# vector of a region padded at every length); 52 500: mean 48.1, sigma 6.9 -- regions that end one entry short of a
# chunk (47), on its boundary (48) and 1, 2, 3, 5, 6 entries past it (49 ..), by the thousand each.
@pytest.mark.parametrize("n", [300, 3_300, 52_500])
def test_tail_shapes(bf, monkeypatch, n):
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    reads = bf.synth_reads_device(23, 0, n, L)
    a, b = insert_both(bf, 1 << 31, reads)
    q = torch.cat([reads, bf.synth_reads_device(24, 0, max(n // 10, 50), L)])
    clean, hits = query_both(a, b, q)
    assert n * 120 <= hits < clean


def test_skewed_input_late_entries_and_overflows(bf, monkeypatch):
    """10^5 reads that are poly-A or copies of one read, among ordinary ones: a handful of segments receive everything.
    A round then offers one ring more than the 48 entries it holds (late entries), more than two rings (overflow), and
    the regions of those segments run over their capacity (packed chunks unpacked into the overflow path)."""
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    n = 160_000
    reads = bf.synth_reads_device(25, 0, n, L).view(n, L)
    reads[20_000:70_000] = ord("A")
    reads[90_000:140_000] = reads[3].clone()
    reads = reads.reshape(-1)
    a, b = insert_both(bf, 1 << 31, reads)
    q = torch.cat([reads[: 30_000 * L], bf.synth_reads_device(26, 0, 5_000, L), reads[85_000 * L: 100_000 * L]])
    query_both(a, b, q)


def test_no_power_of_two_bins_of_whole_segments(bf, monkeypatch):
    """3 * 2^29 bits: 3072 segments as 4 bins of 768 segments, split 768 ways (one-chunk rings, 256 of them unused)"""
    import torch

    monkeypatch.setenv("BTLBF_SPLIT_BITS", "10")
    n = 200_000
    reads = bf.synth_reads_device(27, 0, n, L)
    a, b = insert_both(bf, 3 << 29, reads)
    q = torch.cat([reads[: 20_000 * L], bf.synth_reads_device(28, 0, 20_000, L)])
    clean, hits = query_both(a, b, q)
    assert 20_000 * 120 <= hits < clean - 19_000 * 120


def test_128_kib_segments_20_bit_entries_at_2p39_bits(bf):
    """the benchmark's geometry: 2^19 segments of 128 KiB as 512 bins x 1024 ways, 20-bit entries (bit 19 in use)"""
    import torch

    bits, n = 1 << 39, 2_000_000
    require_hbm(2 * (bits // 8) + (40 << 30), "two filters of 2^39 bits")
    reads = bf.synth_reads_device(29, 0, n, L)
    a, b = insert_both(bf, bits, reads, scratch=16 << 30)
    q = torch.cat([reads[: 100_000 * L], bf.synth_reads_device(30, 0, 20_000, L)])
    clean, hits = query_both(a, b, q)
    assert 100_000 * 120 <= hits < clean - 19_000 * 120
