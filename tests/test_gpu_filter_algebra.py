"""The filter algebra on the GPU (btlbf_clone / btlbf_combine / btlbf_fold / btlbf_threshold_bits; csrc/host_algebra.cpp
over csrc/algebra_kernels.hip) against tests/filter_algebra_model.py (pinned to oracle-built filters by
test_filter_algebra_model_cpu.py), and its three identities through the real pipeline: the union of two built filters is
the filter built from both inputs, a filter folds into the filter built at the smaller size, and the thresholded counting
filter answers contains() as the counting filter does.  Every expectation is exact.  The shapes are those at which the
kernels can go wrong: bodies shorter than a vector, ragged tails, slices at every byte alignment, a grid-stride loop
that wraps (the launchers use at most 4096 blocks of 256 threads, one 16-byte vector per thread and trip), counters next
to their maximum.  The C ABI's threshold is an `unsigned`, so "MAX" for 64-bit counters is 2^32 - 1 here."""
import ctypes as C

import numpy as np
import pytest

import filter_algebra_model as fm

pytestmark = pytest.mark.gpu

MiB = 1 << 20
H, K = 3, 25
WRAP = 4096 * 256 * 16  # bytes one trip of a full grid covers
assert WRAP == 16 * MiB
KINDS = [0, 1, 2, 4, 8]  # counter bytes; 0 = bit filter
OPS = {0: fm.BIT_OPS, 1: fm.COUNTER_OPS, 2: fm.COUNTER_OPS, 4: fm.COUNTER_OPS, 8: fm.COUNTER_OPS}
N_SRCS = [1, 2, 3, 5, 16]
EINVAL = 1


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    return m


def make(m, cb, nbytes, h=H, k=K, thr=0):
    if cb == 0:
        return m.BloomFilter(nbytes * 8, h, k)
    return m.CountingBloomFilter(nbytes, h, k, countThreshold=thr, counter_bits=8 * cb)


def pop(f):
    return f.getPop() if hasattr(f, "getPop") else f.popCount()


def edge_values(cb):
    mx = fm.counter_max(cb)
    return [0, 1, mx - 1, mx]


def saturation_block(cb):
    """(dst counters, src counters): every pair from {0, 1, MAX - 1, MAX}; for 64-bit counters also pairs whose sum carries
    across the 32-bit halves; for bytes the pattern FF 00 01 FF (a saturating counter next to an empty one)"""
    e = edge_values(cb)
    a = [x for x in e for _ in e]
    b = [y for _ in e for y in e]
    if cb == 8:
        a += [0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0x00000001FFFFFFFF]
        b += [0x0000000000000001, 0x0000000100000000, 0x8000000000000001, 0x0000000000000001, 0xFFFFFFFE00000001]
    if cb == 1:
        a += [0xFF, 0x00, 0x01, 0xFF, 0xFF, 0x00, 0x01, 0xFF]
        b += [0x01, 0x00, 0xFF, 0xFF, 0xFF, 0x01, 0x01, 0x00]
    dt = "<u%d" % cb
    return np.array(a, dtype=dt), np.array(b, dtype=dt)


def random_body(rng, cb, nbytes):
    """random contents; counting filters: a third of the counters near MAX, a third zero (so sums saturate, and so
    the popcount is not the counter count)"""
    if cb == 0:
        return rng.integers(0, 256, nbytes, dtype=np.uint8)
    n = nbytes // cb
    mx = fm.counter_max(cb)
    v = rng.integers(0, 4, n, dtype=np.uint64)
    kind = rng.integers(0, 3, n)
    out = np.where(kind == 0, np.uint64(0), np.where(kind == 1, v, np.uint64(mx) - v)).astype("<u%d" % cb)
    return out.view(np.uint8)


def operands(rng, cb, nbytes):
    """17 bodies: [0] is dst, [1:] the sources; dst and the first source begin with the saturation block"""
    bodies = [random_body(rng, cb, nbytes) for _ in range(17)]
    if cb:
        a, b = saturation_block(cb)
        n = min(len(a), nbytes // cb)
        bodies[0].view(a.dtype)[:n] = a[:n]
        bodies[1].view(a.dtype)[:n] = b[:n]
    return bodies


def check_combined(m, dst, got_pop, want_body, want_pop):
    assert got_pop == want_pop == pop(dst)
    assert (dst.download() == want_body).all()
    assert dst.digest() == m.engine.body_digest(want_body)  # the padding behind the body is still zero


# ---- combine against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 16, 24, 4104])
@pytest.mark.parametrize("cb", KINDS)
def test_combine_small(bf, cb, nbytes):
    rng = np.random.default_rng(1000 * cb + nbytes)
    bodies = operands(rng, cb, nbytes)
    srcs = [make(bf, cb, nbytes) for _ in range(16)]
    for f, b in zip(srcs, bodies[1:]):
        f.upload(b)
    dst = make(bf, cb, nbytes)
    for op in OPS[cb]:
        for n in N_SRCS:
            dst.upload(bodies[0])
            got = dst.combine(srcs[:n], op)
            want, want_pop = fm.combine(bodies[0], bodies[1 : 1 + n], op, cb)
            check_combined(bf, dst, got, want, want_pop)


@pytest.mark.parametrize("op_index", [0, 1, 2])
@pytest.mark.parametrize("cb", KINDS)
def test_combine_past_a_grid_wrap_with_a_ragged_tail(bf, cb, op_index):
    nbytes = WRAP + 24
    op = OPS[cb][op_index]
    rng = np.random.default_rng(77 + cb)
    bodies = operands(rng, cb, nbytes)
    srcs = [make(bf, cb, nbytes) for _ in range(16)]
    for f, b in zip(srcs, bodies[1:]):
        f.upload(b)
    dst = make(bf, cb, nbytes)
    for n in N_SRCS:
        dst.upload(bodies[0])
        got = dst.combine(srcs[:n], op)
        want, want_pop = fm.combine_fast(bodies[0], bodies[1 : 1 + n], op, cb)
        check_combined(bf, dst, got, want, want_pop)


@pytest.mark.parametrize("cb", KINDS)
def test_combine_with_operands_that_were_never_touched(bf, cb):
    """created and never touched = lazily cleared: as dst, and as a source"""
    nbytes = 4104
    rng = np.random.default_rng(5 + cb)
    body = random_body(rng, cb, nbytes)
    zero = np.zeros(nbytes, np.uint8)
    for op in OPS[cb]:
        a = make(bf, cb, nbytes)
        a.upload(body)
        dst = make(bf, cb, nbytes)  # lazy dst
        got = dst.combine([a], op)
        check_combined(bf, dst, got, *fm.combine(zero, [body], op, cb))
        dst = make(bf, cb, nbytes)
        dst.upload(body)
        got = dst.combine([a, make(bf, cb, nbytes)], op)  # lazy source
        check_combined(bf, dst, got, *fm.combine(body, [body, zero], op, cb))


def test_copy_is_a_second_filter(bf):
    rng = np.random.default_rng(3)
    for cb in KINDS:
        f = make(bf, cb, 4104, thr=2 if cb else 0)
        lazy = f.copy()
        assert (lazy.download() == 0).all() and lazy.header() == f.header()
        body = random_body(rng, cb, 4104)
        f.upload(body)
        g = f.copy()
        assert type(g) is type(f) and g._h.value != f._h.value
        assert (g.download() == body).all() and g.digest() == f.digest() and g.header() == f.header()
        assert f.compare(g) == (0, 0, 0)
        g.clear()
        assert (f.download() == body).all()  # not shared
    s = bf.BloomFilter.shard(1 << 16, 1, 4, H, K)
    s.upload(random_body(rng, 0, s.localBytes()))
    assert s.copy().digest() == s.digest()  # a shard's digest depends on where the shard starts


# ---- the identities through the real pipeline -------------------------------------------------------------------------
L_READ = 100


def reads_of(bf, seed, n):
    return bf.synth_reads_device(seed, 0, n, L_READ)


SEEDS = ["1111111111110111111111111", "1111111111011111111111111", "1011111111111111111111101"]


@pytest.mark.parametrize("spaced", [False, True])
def test_union_is_the_filter_built_from_both_inputs(bf, spaced):
    import torch

    bits = 1 << 20
    r1, r2 = reads_of(bf, 11, 300), reads_of(bf, 12, 200)

    def new():
        f = bf.BloomFilter(bits, H, K)
        if spaced:
            f.setSpacedSeeds(SEEDS, 1)
        return f

    a, b, both = new(), new(), new()
    a.insertSeqs(r1, read_len=L_READ)
    b.insertSeqs(r2, read_len=L_READ)
    both.insertSeqs(torch.cat([r1, r2]), read_len=L_READ)
    assert a.union(b) is a
    assert a.compare(both) == (0, 0, 0) and a.digest() == both.digest()
    c = new()
    c |= b
    assert c.compare(b) == (0, 0, 0)
    assert (b | c).compare(b) == (0, 0, 0)
    if spaced:  # one refused call: seeds that differ
        other = bf.BloomFilter(bits, H, K)
        other.setSpacedSeeds(SEEDS[:2] + ["1111111110111111111111111"], 1)
        before = a.digest()
        with pytest.raises(Exception, match="spaced seeds"):
            a.union(other)
        with pytest.raises(Exception, match="spaced seeds"):
            a.union(bf.BloomFilter(bits, H, K))
        assert a.digest() == before


@pytest.mark.parametrize("bits_per_counter", [8, 16])
def test_add_merge_is_increment_all_of_both_inputs(bf, bits_per_counter):
    import torch

    nbytes = 1 << 18
    one = reads_of(bf, 21, 1)
    r1 = torch.cat([reads_of(bf, 22, 100)] + [one] * 300)  # 300 copies: byte counters saturate, 16-bit ones do not
    r2 = torch.cat([reads_of(bf, 23, 50), one, one])

    def new():
        return bf.CountingBloomFilter(nbytes, H, K, counter_bits=bits_per_counter)

    a, b, both = new(), new(), new()
    a.insertSeqs(r1, read_len=L_READ, increment_all=True)
    b.insertSeqs(r2, read_len=L_READ, increment_all=True)
    both.insertSeqs(torch.cat([r1, r2]), read_len=L_READ, increment_all=True)
    top = int(both.counters().max())
    assert top == 255 if bits_per_counter == 8 else top >= 302
    assert a.merge(b, op="add") is a
    assert a.compare(both) == (0, 0, 0)


def test_intersect_and_subtract_answer_like_the_model(bf, oracle):
    bits = 1 << 16
    r1, r2 = reads_of(bf, 31, 60), reads_of(bf, 32, 60)
    q = np.concatenate([r1.cpu().numpy(), r2.cpu().numpy(), reads_of(bf, 33, 20).cpu().numpy()])
    a, b = bf.BloomFilter(bits, H, K), bf.BloomFilter(bits, H, K)
    a.insertSeqs(r1, read_len=L_READ)
    b.insertSeqs(r2, read_len=L_READ)
    a.insertSeqs(r2[: 20 * L_READ], read_len=L_READ)
    ab, bb = a.download(), b.download()
    for method, op in (("intersect", fm.AND), ("subtract", fm.ANDNOT)):
        c = a.copy()
        getattr(c, method)(b)
        body, _ = fm.combine(ab, [bb], op, 0)
        assert (c.download() == body).all()
        hit, _, _ = c.containsSeqs(q, read_len=L_READ)
        want = []
        for r in q.reshape(-1, L_READ):
            h, _ = oracle.bf_contains_seq_dense(body, bits, H, K, r.tobytes())
            want.append(np.concatenate([h, np.zeros(K - 1, np.uint8)]))
        assert (bf.bits_to_bool(hit, len(q)) == np.concatenate(want).astype(bool)).all()
    assert (a & b).compare(a.copy().intersect(b)) == (0, 0, 0)
    assert (a - b).compare(a.copy().subtract(b)) == (0, 0, 0)


def test_combine_refuses_what_does_not_fit(bf):
    a = bf.BloomFilter(1 << 12, H, K)
    a.upload(np.full(512, 0x5A, np.uint8))
    before = a.digest()
    c8 = bf.CountingBloomFilter(512, H, K)
    for others, op, word in (([a], "or", "among the sources"), ([], "or", "n_srcs"), ([c8], "or", "kind"),
                             ([bf.BloomFilter(1 << 13, H, K)], "or", "size"), ([bf.BloomFilter(1 << 12, H + 1, K)], "or", "hash_num"),
                             ([bf.BloomFilter(1 << 12, H, K + 1)], "and", "kmer_size"), ([bf.BloomFilter(1 << 12, H, K)], "add", "op"),
                             ([bf.BloomFilter(1 << 12, H, K)] * 17, "or", "n_srcs")):
        with pytest.raises(Exception, match=word):
            a.combine(others, op)
    with pytest.raises(Exception, match="op"):
        c8.combine([bf.CountingBloomFilter(512, H, K)], "or")
    with pytest.raises(Exception, match="kind"):
        c8.combine([bf.CountingBloomFilter(512, H, K, counter_bits=16)], "add")
    assert a.digest() == before


# ---- fold ---------------------------------------------------------------------------------------------------------------
def check_fold(bf, cb, slice_bytes, factor, rng, thr=0):
    body = random_body(rng, cb, slice_bytes * factor)
    f = make(bf, cb, slice_bytes * factor, thr=thr)
    f.upload(body)
    if cb == 0:
        f.setnEntry(12345)
    g = f.fold(factor)
    want = fm.fold(body, factor, cb)
    assert want.size == slice_bytes
    assert (g.download() == want).all()
    assert g.digest() == bf.engine.body_digest(want)  # the padding behind the body is zero
    small = make(bf, cb, slice_bytes, thr=thr)
    if cb == 0:
        small.setnEntry(12345)  # (carried over)
    assert g.header() == small.header() and g.localBytes() == small.localBytes() == slice_bytes
    assert g.getHashNum() == H and g.getKmerSize() == K
    assert type(g) is type(f)
    if cb:
        assert g.threshold() == thr and g.size() == small.size() and g.counterBytes() == cb
    else:
        assert g.getFilterSize() == 8 * slice_bytes
    assert (f.download() == body).all()  # the source is as it was


@pytest.mark.parametrize("factor", [2, 3, 5, 64, 1000])
@pytest.mark.parametrize("slice_bytes", [1, 7, 8, 9, 15, 16, 17, 4099])
def test_fold_bit_filter_at_every_alignment(bf, slice_bytes, factor):
    check_fold(bf, 0, slice_bytes, factor, np.random.default_rng(slice_bytes * 1009 + factor))


def test_fold_small_result_large_factor_takes_two_stages(bf):
    check_fold(bf, 0, 24, 65536, np.random.default_rng(24))


def test_fold_large_result(bf):
    check_fold(bf, 0, MiB + 8, 3, np.random.default_rng(8))


@pytest.mark.parametrize("factor", [2, 3, 64, 4096])
@pytest.mark.parametrize("slice_bytes", [8, 24, 4104])
@pytest.mark.parametrize("cb", [1, 2, 4, 8])
def test_fold_counting_filter_saturates(bf, cb, slice_bytes, factor):
    check_fold(bf, cb, slice_bytes, factor, np.random.default_rng(cb * 7919 + slice_bytes + factor), thr=3)


def test_fold_by_one_is_a_copy_and_refusals(bf):
    f = bf.BloomFilter(1 << 12, H, K)
    body = random_body(np.random.default_rng(1), 0, 512)
    f.upload(body)
    assert (f.fold(1).download() == body).all()
    for factor, word in ((0, "at least 1"), (3, "does not divide"), (1 << 10, "multiple of 8"), (1 << 13, "does not divide")):
        with pytest.raises(Exception, match=word):
            f.fold(factor)
    c = bf.CountingBloomFilter(64, H, K, counter_bits=16)
    with pytest.raises(Exception, match="multiple of 8"):
        c.fold(16)  # 2 counters of 2 bytes
    with pytest.raises(Exception, match="shard"):
        bf.BloomFilter.shard(1 << 16, 0, 4, H, K).fold(2)


@pytest.mark.parametrize("cb", KINDS)
def test_folded_filter_is_the_filter_built_at_the_smaller_size(bf, cb):
    """insertSeqs / incrementAll at m and at m / 6, from the same reads"""
    factor, small_bytes = 6, 40 * 1024 + 8
    reads = reads_of(bf, 41 + cb, 400)
    big, small = make(bf, cb, small_bytes * factor), make(bf, cb, small_bytes)
    for f in (big, small):
        if cb:
            f.insertSeqs(reads, read_len=L_READ, increment_all=True)
        else:
            f.insertSeqs(reads, read_len=L_READ)
    g = big.fold(factor)
    assert pop(small) > 0 and g.compare(small) == (0, 0, 0) and g.digest() == small.digest()


# ---- threshold --------------------------------------------------------------------------------------------------------
def counters_with_edges(rng, cb, n, t_max):
    """n counters: values around 1, 2 and the largest threshold, and zeros"""
    pool = np.array([0, 0, 1, 2, 3, t_max - 1, t_max, fm.counter_max(cb)], dtype="<u%d" % cb)
    return pool[rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("n_counters", [8, 72, "wrap"])
@pytest.mark.parametrize("cb", [1, 2, 4, 8])
def test_threshold_bits(bf, cb, n_counters):
    t_max = min(fm.counter_max(cb), (1 << 32) - 1)
    n = WRAP // cb + 72 if n_counters == "wrap" else n_counters
    rng = np.random.default_rng(cb * 31 + n % 1000)
    c = counters_with_edges(rng, cb, n, t_max)
    f = make(bf, cb, n * cb, thr=2)
    f.upload(c.view(np.uint8))
    for t in (1, 2, t_max):
        b = f.toBloomFilter(t)
        want = np.packbits(c >= c.dtype.type(t), bitorder="little")
        assert isinstance(b, bf.BloomFilter) and b.getFilterSize() == n and b.localBytes() == n // 8
        assert (b.download() == want).all() and (want == fm.threshold_bits(c.view(np.uint8), t, cb)).all()
        assert b.digest() == bf.engine.body_digest(want)  # the last partial word and the padding are zero
        assert b.getPop() == int((c >= c.dtype.type(t)).sum())
        assert b.getHashNum() == H and b.getKmerSize() == K and b.getnEntry() == 0
    assert f.toBloomFilter().compare(f.toBloomFilter(2)) == (0, 0, 0)  # default: the filter's own threshold
    if cb < 4:  # a threshold no counter of this width reaches
        assert f.toBloomFilter(t_max + 1).getPop() == 0


@pytest.mark.parametrize("cb", [1, 2, 4, 8])
def test_thresholded_filter_answers_like_the_counting_filter(bf, cb):
    import torch

    once, twice = reads_of(bf, 51, 80), reads_of(bf, 52, 80)
    nbytes = 1 << 16
    for t in (1, 2, 3):
        f = make(bf, cb, nbytes, thr=t)
        f.insertSeqs(torch.cat([once, twice, twice]), read_len=L_READ, increment_all=True)
        q = torch.cat([once, twice, reads_of(bf, 53, 40)])
        hit_c, valid_c, _ = f.containsSeqs(q, read_len=L_READ)
        hit_b, valid_b, _ = f.toBloomFilter().containsSeqs(q, read_len=L_READ)
        assert torch.equal(hit_c, hit_b) and torch.equal(valid_c, valid_b)
        assert int(hit_c.ne(0).sum()) > 0


def test_threshold_refusals(bf):
    with pytest.raises(Exception, match="counting filter"):
        C_h = C.c_void_p()
        f = bf.BloomFilter(1 << 12, H, K)
        bf.engine.check(f._L.btlbf_threshold_bits(C.byref(C_h), f._h, 1))
    with pytest.raises(Exception, match="threshold"):
        bf.CountingBloomFilter(64, H, K).toBloomFilter()
    with pytest.raises(Exception, match="multiple of 8"):
        bf.CountingBloomFilter(8, H, K, counter_bits=16, countThreshold=1).toBloomFilter()  # 4 counters
