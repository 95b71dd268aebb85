"""The device-side judges against ground truth.  Almost every parity test of the partitioned pipeline ends in
`b.compare(a) == (0, 0, 0)`, `a.digest() == b.digest()` or `a.getPop() == b.getPop()`: btlbf_compare, btlbf_digest and
btlbf_popcount / btlbf_filtered_popcount / btlbf_popcount_bits (csrc/host_aux.cpp over compare_kernel, digest_kernel and
popcount_kernel in csrc/aux_kernels.hip) decide in HBM what cannot be downloaded.  Here they are measured themselves:
against tests/judge_model.py (pinned on the host by test_judge_model_cpu.py) on dense arrays that are downloaded truth,
on one planted difference in every position class of the grid-stride loops, on sparse arrays past every 32-bit mark of
a byte offset or vector index (cleared and scanned, never filled), on shards, and after a pending clear.  Every
expectation is an exact integer."""
import ctypes as C
import functools

import numpy as np
import pytest
from conftest import require_hbm

import judge_model as jm

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
# One trip of every thread through the grid-stride loop, from the launchers in csrc/aux_kernels.hip:
#   launch_popcount (:310-314) and launch_compare (:414-418): at most 4096 blocks x 256 threads x one uint2 (8 B)
#   launch_digest (:360-363): at most 8192 blocks x 256 threads x one uint4 (16 B)
COMPARE_STRIDE = POPCOUNT_STRIDE = 4096 * 256 * 8
DIGEST_STRIDE = 8192 * 256 * 16
assert COMPARE_STRIDE == 8 * MiB and DIGEST_STRIDE == 32 * MiB
WAVE = 64
OK, EINVAL = 0, 1
SENTINEL = 0xA5A5A5A5A5A5A5A5  # what an output holds before a call that must not write it
H, K = 3, 25  # hash count and k: the judges do not look at either


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    return m


# ---- harness: the C ABI where the Python classes have no method ---------------------------------------------------
def _upload_at(lib, f, offset, data):
    buf = bytes(data)
    assert lib.btlbf_upload(f._h, buf, offset, len(buf)) == OK, lib.btlbf_last_error()


def _download_at(lib, f, offset, nbytes):
    out = C.create_string_buffer(nbytes)
    assert lib.btlbf_download(f._h, out, offset, nbytes) == OK, lib.btlbf_last_error()
    return out.raw


def _counting_shard(lib, size, index, count, thr):
    """btlbf_create_shard for a counting filter, as a CountingBloomFilter object (the class has no shard constructor)"""
    from btl_bloomfilter_amd import _lib, engine

    h = C.c_void_p()
    _lib.check(lib.btlbf_create_shard(C.byref(h), _lib.COUNTING8, size, index, count, H, K, thr, 0))
    f = engine.CountingBloomFilter.__new__(engine.CountingBloomFilter)
    engine._Filter.__init__(f, h)
    return f


def _pop(f):
    return f.popCount() if hasattr(f, "popCount") else f.getPop()


def _close(*filters):
    for f in filters:
        f.close()


@functools.lru_cache(maxsize=None)
def _pair(n):
    """two bodies of n bytes, computed once and shared read-only: x is random with long zero runs, y equals x except
    in about 1000 random bytes"""
    rng = np.random.default_rng(n)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    run = 4096 if n >= MiB else 32
    x[np.repeat(rng.random((n + run - 1) // run) < 0.5, run)[:n]] = 0
    x[n - 1] |= 0x81  # the last local byte is never empty
    y = x.copy()
    idx = np.unique(rng.integers(0, n, min(1000, max(1, n // 3))))
    y[idx] = rng.integers(0, 256, idx.size, dtype=np.uint8)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _truth(n):
    """the model's answers for _pair(n), computed once"""
    from btl_bloomfilter_amd.engine import body_digest

    x, y = _pair(n)
    return {"dx": body_digest(x), "dy": body_digest(y),
            "bits": jm.dense_compare(x, y, False), "counters": jm.dense_compare(x, y, True)}


# ---- A. dense arrays, downloaded truth -------------------------------------------------------------------------------
# local sizes in bytes: a padded last word; a padded last word above 64 KiB; one stride plus three vectors (padded to
# 16); three strides and an odd tail; above the digest's stride
DENSE_SIZES = [125, 100_001, 8 * MiB + 24, 25 * MiB + 8, 80 * MiB + 16]


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_bit_filter_judges_equal_the_model_on_dense_arrays(bf, n):
    x, y = _pair(n)
    t = _truth(n)
    a, b = bf.BloomFilter(8 * n, H, K), bf.BloomFilter(8 * n, H, K)
    try:
        assert a.localBytes() == b.localBytes() == n
        a.upload(x)
        b.upload(y)
        assert (a.download() == x).all() and (b.download() == y).all()
        differ, a_only, b_only = t["bits"]
        assert differ == a_only + b_only and a_only > 0 and b_only > 0
        assert a.compare(b) == (differ, a_only, b_only)
        assert b.compare(a) == (differ, b_only, a_only)
        assert a.compare(a) == (0, 0, 0) == b.compare(b)
        assert a.digest() == t["dx"] and b.digest() == t["dy"] and t["dx"] != t["dy"]
        assert a.getPop() == jm.dense_popcount(x, 0) > 0
        assert b.getPop() == jm.dense_popcount(y, 0) > 0
    finally:
        _close(a, b)


@pytest.mark.parametrize("n", DENSE_SIZES)
def test_counting_filter_judges_equal_the_model_on_dense_arrays(bf, n):
    """a counting filter's size is rounded up to 8 bytes (125 -> 128, 100 001 -> 100 008); 100 008, 8 MiB + 24 and
    25 MiB + 8 are allocated with 8 bytes of zero padding, which `counter >= 0` must not count"""
    local = -(-n // 8) * 8
    x, y = _pair(local)
    t = _truth(local)
    by_thr = {thr: bf.CountingBloomFilter(n, H, K, thr) for thr in (0, 1, 2, 200, 255)}
    b = bf.CountingBloomFilter(n, H, K, 2)
    try:
        a = by_thr[1]
        for f in by_thr.values():
            assert f.localBytes() == local
            f.upload(x)
        b.upload(y)
        assert (a.download() == x).all() and (b.download() == y).all()
        differ, greater, less = t["counters"]
        assert differ == greater + less and greater > 0 and less > 0
        assert a.compare(b) == (differ, greater, less)
        assert b.compare(a) == (differ, less, greater)
        assert a.compare(a) == (0, 0, 0) == b.compare(b)
        assert a.digest() == t["dx"] and b.digest() == t["dy"] and t["dx"] != t["dy"]
        for thr, f in by_thr.items():
            assert f.threshold() == thr
            assert f.popCount() == jm.dense_popcount(x, 1) > 0
            assert f.filtered_popcount() == jm.dense_popcount(x, 2, thr), "threshold %d" % thr
        assert by_thr[0].filtered_popcount() == local
        assert b.popCount() == jm.dense_popcount(y, 1) and b.filtered_popcount() == jm.dense_popcount(y, 2, 2)
    finally:
        _close(b, *by_thr.values())


def test_popcount_bits_of_a_raw_device_buffer_equals_the_model(bf, lib):
    """btlbf_popcount_bits judges the query bitmaps of the big tests: whole uint64 words of raw device memory, below,
    at and above one stride; a byte count that is no multiple of 8 is an error, never a count"""
    import torch

    x, _ = _pair(80 * MiB + 16)
    dev = torch.from_numpy(x.copy()).cuda()
    torch.cuda.synchronize()
    first = int(np.flatnonzero(x)[0]) // 8 * 8  # a word that is not inside a zero run
    assert first > 0

    def bits(start, nbytes):
        out = C.c_uint64(SENTINEL)
        rc = lib.btlbf_popcount_bits(C.c_void_p(dev.data_ptr() + start), nbytes, C.byref(out), 0, None)
        return rc, out.value

    for n in (8, 120, POPCOUNT_STRIDE - 8, POPCOUNT_STRIDE, POPCOUNT_STRIDE + 8, 8 * MiB + 24, 25 * MiB + 8, 80 * MiB + 16):
        for start in (0, first):
            if start + n <= x.size:
                assert bits(start, n) == (OK, jm.dense_popcount(x[start: start + n], 0)), (start, n)
    assert bits(first, 120)[1] > 0
    assert bits(0, 0) == (OK, 0)
    for n in (1, 7, 125, POPCOUNT_STRIDE + 4, 100_001):
        assert bits(first, n) == (EINVAL, SENTINEL), n


# ---- B. one planted difference, every position class ----------------------------------------------------------------
PLANTED_LOCAL = 25 * MiB + 8


def _position_classes(n):
    offs = {0, 7, 8, 15, 16, n - 1}
    for stride in (COMPARE_STRIDE, DIGEST_STRIDE):
        for edge in range(stride, n, stride):  # the last byte before each stride boundary and the first after it
            offs |= {edge - 1, edge}
    # 64 consecutive vectors from a stride boundary: every lane of a wave is once the only one that sees a difference,
    # for the uint2 kernels and for the digest's uint4 (both words of its vector)
    offs |= {COMPARE_STRIDE + 8 * j + j % 8 for j in range(WAVE)}
    offs |= {COMPARE_STRIDE + 16 * j + (5 * j + 3) % 16 for j in range(WAVE)}
    offs |= {2 * COMPARE_STRIDE + 8 * j for j in range(WAVE)}
    assert all(0 <= o < n for o in offs)
    return sorted(offs)


@pytest.mark.parametrize("counting", [False, True], ids=["bits", "counters"])
def test_one_planted_difference_in_every_position_class(bf, lib, counting):
    """a is random, b = a except ONE byte (one bit flipped / one counter moved by 1), changed through
    btlbf_upload(offset, 1): compare is exactly (1, 1, 0) or (1, 0, 1), the popcounts move by the model's amount, the
    digest is the definition's"""
    from btl_bloomfilter_amd.engine import body_digest

    n = PLANTED_LOCAL
    x, _ = _pair(n)
    if counting:
        a, b = bf.CountingBloomFilter(n, H, K, 2), bf.CountingBloomFilter(n, H, K, 2)
    else:
        a, b = bf.BloomFilter(8 * n, H, K), bf.BloomFilter(8 * n, H, K)
    try:
        assert a.localBytes() == n
        a.upload(x)
        b.upload(x)
        mode = 1 if counting else 0
        d0, pop0 = _truth(n)["dx"], jm.dense_popcount(x, mode)
        fpop0 = jm.dense_popcount(x, 2, 2)
        assert a.digest() == b.digest() == d0 and _pop(a) == _pop(b) == pop0 and a.compare(b) == (0, 0, 0)
        words = x.view("<u8")
        offsets = _position_classes(n)
        bad, seen, moved = [], set(), set()
        for i, off in enumerate(offsets):
            old = int(x[off])
            if counting:
                new = old - 1 if old == 255 or (old > 0 and i % 2) else old + 1
            else:
                new = old ^ (1 << (i % 8))
            triple = jm.sparse_compare({off: old}, {off: new}, counting)
            assert triple in ((1, 1, 0), (1, 0, 1))
            old_w = int(words[off >> 3])
            new_w = old_w ^ ((old ^ new) << (8 * (off & 7)))
            want_d = jm.digest_with_word_replaced(d0, off >> 3, old_w, new_w)
            assert want_d != d0
            if off in (0, n - 1):  # the incremental form is the definition: tie it to body_digest on the device's bytes
                z = x.copy()
                z[off] = new
                assert want_d == body_digest(z)
            want_pop = pop0 + jm.dense_popcount([new], mode) - jm.dense_popcount([old], mode)
            want = [triple, (triple[0], triple[2], triple[1]), want_pop, want_d]
            _upload_at(lib, b, off, [new])
            got = [a.compare(b), b.compare(a), _pop(b), b.digest()]
            if counting:
                want.append(fpop0 + (new >= 2) - (old >= 2))
                got.append(b.filtered_popcount())
            _upload_at(lib, b, off, [old])
            seen.add(triple)
            moved.add(want_pop - pop0)
            if got != want:
                bad.append((off, got, want))
        assert not bad, "%d of %d offsets, first (offset, got, want): %r" % (len(bad), len(offsets), bad[:3])
        assert seen == {(1, 1, 0), (1, 0, 1)}
        if not counting:
            assert moved == {-1, 1}
        assert a.compare(b) == (0, 0, 0) and b.digest() == d0  # every byte was put back
    finally:
        _close(a, b)


# ---- C. sparse arrays past the 32-bit marks, no download -------------------------------------------------------------
def _marks(local):
    """byte offsets of the planted 8-byte values: around bit 2^32, byte 2^32, uint2 vector 2^32 (byte 2^35) and uint4
    vector 2^32 (byte 2^36, both words of the vector before it), and the two ends -- where the array reaches them"""
    cands = [0, 2 ** 29 - 8, 2 ** 29, 2 ** 32 - 8, 2 ** 32, 2 ** 35 - 8, 2 ** 35, 2 ** 36 - 16, 2 ** 36 - 8, 2 ** 36, local - 8]
    return sorted({m for m in cands if m + 8 <= local})


def _plant_on_device(lib, f, planted, offset, data):
    _upload_at(lib, f, offset, data)
    jm.plant(planted, offset, data)


def _verify_planted(lib, f, planted):
    """a failed upload is not to be blamed on a judge"""
    for w in sorted({off >> 3 for off in planted}):
        want = bytes(planted.get(8 * w + j, 0) for j in range(8))
        assert _download_at(lib, f, 8 * w, 8) == want, "planted bytes at offset %d" % (8 * w)


def _value(rng, counting):
    v = rng.integers(1, 256, 8, dtype=np.uint8)
    if counting:
        v[:4] = rng.permutation(np.array([255, 1, 0, 254], np.uint8))  # the thresholds' neighbours; an empty counter
    return bytes(v)


def _plant_pair(lib, a, b, local, counting):
    """around every mark: a word that differs, a word both share, a word only a has, a word only b has"""
    rng = np.random.default_rng(local % 1009)
    pa, pb = {}, {}
    for m in _marks(local):
        va, vb = _value(rng, counting), _value(rng, counting)
        assert va != vb
        _plant_on_device(lib, a, pa, m, va)
        _plant_on_device(lib, b, pb, m, vb)
        if m + 200 <= local:
            same, only_a, only_b = _value(rng, counting), _value(rng, counting), _value(rng, counting)
            _plant_on_device(lib, a, pa, m + 64, same)
            _plant_on_device(lib, b, pb, m + 64, same)
            _plant_on_device(lib, a, pa, m + 128, only_a)
            _plant_on_device(lib, b, pb, m + 192, only_b)
    _verify_planted(lib, a, pa)
    _verify_planted(lib, b, pb)
    return pa, pb


def test_sparse_bit_filter_of_72_gib_digest_and_popcount(bf, lib):
    """2^39 + 2^36 bits: the digest's uint4 vector index passes 2^32 at byte 2^36, popcount's uint2 index at 2^35"""
    bits = 2 ** 39 + 2 ** 36
    local = bits // 8
    require_hbm(local + 4 * GiB, "a bit filter of 72 GiB")
    f = bf.BloomFilter(bits, H, K)
    try:
        assert f.localBytes() == local
        f.clear()
        assert f.digest() == (0, 0) and f.getPop() == 0
        rng = np.random.default_rng(72)
        planted = {}
        marks = _marks(local)
        assert {2 ** 35, 2 ** 36 - 16, 2 ** 36, local - 8} <= set(marks)
        for m in marks:
            _plant_on_device(lib, f, planted, m, _value(rng, False))
        _verify_planted(lib, f, planted)
        assert f.digest() == jm.sparse_digest(jm.words_of(planted)) != (0, 0)
        assert f.getPop() == jm.sparse_popcount(planted, 0) > 0
    finally:
        _close(f)


def test_sparse_bit_filter_pair_of_36_gib_compare(bf, lib):
    """2^38 + 2^35 bits each: compare's uint2 vector index passes 2^32 at byte 2^35"""
    bits = 2 ** 38 + 2 ** 35
    local = bits // 8
    require_hbm(2 * local + 4 * GiB, "two bit filters of 36 GiB")
    a, b = bf.BloomFilter(bits, H, K), bf.BloomFilter(bits, H, K)
    try:
        a.clear()
        b.clear()
        assert a.compare(b) == (0, 0, 0)
        assert {2 ** 35 - 8, 2 ** 35, local - 8} <= set(_marks(local))
        pa, pb = _plant_pair(lib, a, b, local, False)
        want = jm.sparse_compare(pa, pb, False)
        assert want[1] > 0 and want[2] > 0
        assert a.compare(b) == want
        assert b.compare(a) == (want[0], want[2], want[1])
        assert a.compare(a) == (0, 0, 0) == b.compare(b)
        for f, p in ((a, pa), (b, pb)):
            assert f.digest() == jm.sparse_digest(jm.words_of(p))
            assert f.getPop() == jm.sparse_popcount(p, 0)
    finally:
        _close(a, b)


def test_sparse_counting_filter_pair_past_byte_2p32(bf, lib):
    """2^32 + 2^29 counters each: byte offsets past 2^32"""
    local = 2 ** 32 + 2 ** 29
    require_hbm(2 * local + 2 * GiB, "two counting filters of 4.5 GiB")
    a, b = bf.CountingBloomFilter(local, H, K, 1), bf.CountingBloomFilter(local, H, K, 255)
    try:
        assert a.localBytes() == local
        a.clear()
        b.clear()
        assert {2 ** 32 - 8, 2 ** 32, local - 8} <= set(_marks(local))
        pa, pb = _plant_pair(lib, a, b, local, True)
        want = jm.sparse_compare(pa, pb, True)
        assert want[1] > 0 and want[2] > 0
        assert a.compare(b) == want
        assert b.compare(a) == (want[0], want[2], want[1])
        assert a.compare(a) == (0, 0, 0) == b.compare(b)
        for f, p, thr in ((a, pa, 1), (b, pb, 255)):
            assert f.digest() == jm.sparse_digest(jm.words_of(p))
            assert f.popCount() == jm.sparse_popcount(p, 1) > 0
            assert f.filtered_popcount() == jm.sparse_popcount(p, 2, thr) > 0
        assert a.filtered_popcount() == a.popCount() > b.filtered_popcount()
    finally:
        _close(a, b)


# ---- D. shards and pending clears -------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True], ids=["bits", "counters"])
def test_shard_judges_are_local_and_digests_combine(bf, lib, counting):
    """four shards of a 2^30-bit / 2^27-counter filter (32 MiB each, the digest's stride) with random bodies"""
    from btl_bloomfilter_amd.engine import body_digest

    W, local = 4, 32 * MiB
    size = W * local * (1 if counting else 8)
    per_word = 8 if counting else 64
    first, other = _pair(local)  # other differs from shard 0's body in about 1000 bytes
    whole_body = np.concatenate([np.roll(first, 4099 * r) for r in range(W)])

    def shard(r, thr=2):
        return _counting_shard(lib, size, r, W, thr) if counting else bf.BloomFilter.shard(size, r, W, H, K)

    whole = bf.CountingBloomFilter(size, H, K, 2) if counting else bf.BloomFilter(size, H, K)
    shards = [shard(r) for r in range(W)]
    twin = shard(0)
    try:
        whole.upload(whole_body)
        s = x = 0
        for r, f in enumerate(shards):
            body = whole_body[r * local: (r + 1) * local]
            assert f.localBytes() == local
            f.upload(body)
            ds, dx = f.digest()
            assert (ds, dx) == body_digest(body, first_word=r * (size // W) // per_word)
            if r == 1:
                assert (ds, dx) != body_digest(body)  # the word index is the whole filter's
            assert _pop(f) == jm.dense_popcount(body, 1 if counting else 0) > 0
            if counting:
                assert f.filtered_popcount() == jm.dense_popcount(body, 2, 2)
            s = (s + ds) & jm.M64
            x ^= dx
        assert (s, x) == whole.digest() == body_digest(whole_body)
        twin.upload(other)
        want = jm.dense_compare(whole_body[:local], other, counting)
        assert want == _truth(local)["counters" if counting else "bits"] and want[1] > 0 and want[2] > 0
        assert shards[0].compare(twin) == want
        assert twin.compare(shards[0]) == (want[0], want[2], want[1])
        assert shards[0].compare(shards[0]) == (0, 0, 0)
    finally:
        _close(whole, twin, *shards)


def test_shard_whose_local_byte_count_is_no_multiple_of_16(bf, lib):
    """bit shards of 64 * (2^17 + 1) bits hold 1 MiB + 8 bytes: 8 bytes of padding that no judge may see.  A counting
    shard is a multiple of 64 counters (btlbf_create_shard refuses any other), so its padding correction at threshold
    0 is zero: every local counter counts, once"""
    from btl_bloomfilter_amd import _lib
    from btl_bloomfilter_amd.engine import body_digest

    W, local = 3, MiB + 8
    bits = W * local * 8
    x, y = _pair(local)
    a, b = bf.BloomFilter.shard(bits, 2, W, H, K), bf.BloomFilter.shard(bits, 2, W, H, K)
    c = d = None
    try:
        assert a.localBytes() == local and local % 16 == 8
        a.upload(x)
        b.upload(y)
        assert a.digest() == body_digest(x, first_word=2 * local // 8)
        assert a.getPop() == jm.dense_popcount(x, 0) and b.getPop() == jm.dense_popcount(y, 0)
        assert a.compare(b) == jm.dense_compare(x, y, False)
        # the last local byte, next to the padding
        _upload_at(lib, b, 0, x.tobytes())
        _upload_at(lib, b, local - 1, [int(x[-1]) ^ 0x80])
        assert a.compare(b) == (1, 1, 0) and b.getPop() == a.getPop() - 1 and b.digest() != a.digest()
        clocal = 64 * 16385  # 1 MiB + 64 counters
        cx, cy = _pair(clocal)
        c, d = _counting_shard(lib, W * clocal, 1, W, 0), _counting_shard(lib, W * clocal, 1, W, 255)
        c.upload(cx)
        d.upload(cy)
        assert c.localBytes() == clocal
        assert c.filtered_popcount() == clocal == jm.dense_popcount(cx, 2, 0)
        assert d.filtered_popcount() == jm.dense_popcount(cy, 2, 255) > 0
        assert c.popCount() == jm.dense_popcount(cx, 1)
        assert c.digest() == body_digest(cx, first_word=clocal // 8)
        assert c.compare(d) == jm.dense_compare(cx, cy, True)
        h = C.c_void_p()
        assert lib.btlbf_create_shard(C.byref(h), _lib.COUNTING8, W * (clocal + 8), 1, W, H, K, 0, 0) == EINVAL and not h
    finally:
        _close(*(f for f in (a, b, c, d) if f is not None))


def test_compare_refuses_filters_of_another_kind_size_or_shard_range(bf, lib):
    """EINVAL and no triple: the outputs keep what they held"""
    bits = 1 << 20
    base = bf.BloomFilter(bits, H, K)
    others = {
        "kind": bf.CountingBloomFilter(bits // 8, H, K, 1),            # the same bytes, counters
        "size": bf.BloomFilter(bits + 128, H, K),
        "shard range": bf.BloomFilter.shard(4 * bits, 1, 4, H, K),     # the same local bytes, of a larger filter
    }
    s0, s1 = bf.BloomFilter.shard(4 * bits, 0, 4, H, K), bf.BloomFilter.shard(4 * bits, 1, 4, H, K)
    c0, c1 = _counting_shard(lib, bits, 0, 2, 1), _counting_shard(lib, bits, 1, 2, 1)
    try:
        pairs = [(base, o, what) for what, o in others.items()]
        pairs += [(s0, s1, "shard range"), (c0, c1, "shard range"), (c0, others["kind"], "size")]
        for x, y, what in pairs:
            for p, q in ((x, y), (y, x)):
                out = (C.c_uint64 * 3)(SENTINEL, SENTINEL, SENTINEL)
                assert lib.btlbf_compare(p._h, q._h, out) == EINVAL, what
                assert list(out) == [SENTINEL] * 3, what
        out = (C.c_uint64 * 3)(SENTINEL, SENTINEL, SENTINEL)
        assert lib.btlbf_compare(s1._h, others["shard range"]._h, out) == OK and list(out) == [0, 0, 0]
    finally:
        _close(base, s0, s1, c0, c1, *others.values())


@pytest.mark.parametrize("counting", [False, True], ids=["bits", "counters"])
def test_judges_carry_out_a_pending_clear_themselves(bf, counting):
    """btlbf_clear is lazy: the judge that comes next, with no other call in between, must see an empty array"""
    n = 8 * MiB + 24 if not counting else 8 * MiB + 16
    x, _ = _pair(n)

    def make():
        return bf.CountingBloomFilter(n, H, K, 1) if counting else bf.BloomFilter(8 * n, H, K)

    f, g = make(), make()
    try:
        g.upload(x)
        pop = _pop(g)
        assert pop == jm.dense_popcount(x, 1 if counting else 0) > 0
        f.upload(x)
        f.clear()
        assert f.digest() == (0, 0)
        f.upload(x)
        f.clear()
        assert _pop(f) == 0
        if counting:
            f.upload(x)
            f.clear()
            assert f.filtered_popcount() == 0
        f.upload(x)
        f.clear()
        assert g.compare(f) == (pop, pop, 0)
        f.upload(x)
        f.clear()
        assert f.compare(g) == (pop, 0, pop)
        f.upload(x)
        assert f.compare(g) == (0, 0, 0)
        f.clear()
        g.clear()
        assert f.compare(g) == (0, 0, 0)
        assert (f.download() == 0).all()
    finally:
        _close(f, g)
