"""The slice helper of the AUTO-query GPU tests (auto_query_slices.py), checked on the CPU: its masking of the
windows that straddle two reads against one oracle call per read, its bitmap and window arithmetic against plain
loops."""
import numpy as np
import pytest

from auto_query_slices import bitmap_bits, clean_windows, expected_slice_bits, slice_ranges


def _reads(rng, n, L):
    a = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), size=(n, L))
    a[rng.random((n, L)) < 0.01] = ord("N")
    a[3] = ord("N")  # a read without a clean window
    a[5, 0] = a[5, L - 1] = ord("N")
    return a


@pytest.mark.parametrize("L,k", [(40, 31), (32, 32), (33, 32), (50, 8)])
def test_slice_helper_equals_per_read_oracle_calls_bit_filter(oracle, L, k):
    rng = np.random.default_rng(L * 100 + k)
    bits, h, n = 1 << 16, 3, 300
    a = _reads(rng, n, L)
    body = np.zeros(bits // 8, np.uint8)
    for r in a[::2]:  # every other read is in the filter; the filter is full enough for false positives
        oracle.bf_insert_seq(body, bits, h, k, r.tobytes())
    hit, valid = expected_slice_bits(oracle, body, {"kind": "bf", "bits": bits, "h": h, "k": k}, a.reshape(-1), L)
    assert hit.shape == valid.shape == (n * L,)
    W = L - k + 1
    for i, r in enumerate(a):
        eh, ev = oracle.bf_contains_seq_dense(body, bits, h, k, r.tobytes())
        assert (hit[i * L: i * L + W] == eh).all() and (valid[i * L: i * L + W] == ev).all(), i
        assert not hit[i * L + W: (i + 1) * L].any() and not valid[i * L + W: (i + 1) * L].any(), i
    assert (hit <= valid).all() and 0 < hit.sum() < valid.sum() and not valid[3 * L: 4 * L].any()
    assert valid.sum() == clean_windows(a.reshape(-1), L, k)
    # whole reads only, and an empty slice
    e0, e1 = expected_slice_bits(oracle, body, {"kind": "bf", "bits": bits, "h": h, "k": k}, a[:0].reshape(-1), L)
    assert e0.size == e1.size == 0


def test_slice_helper_equals_per_read_oracle_calls_counting_filter(oracle):
    rng = np.random.default_rng(9)
    L, k, h, n, nbytes = 45, 25, 3, 300, 1 << 14
    a = _reads(rng, n, L)
    body = np.zeros(nbytes, np.uint8)
    for rows in (a, a[: n // 2]):  # the first half is in twice
        for r in rows:
            _, hv = oracle.nthash_seq(r.tobytes(), h, k)
            if len(hv):
                oracle.cbf_increment_all(body, h, hv)
    res = {}
    for thr in (1, 2):
        hit, valid = expected_slice_bits(oracle, body, {"kind": "cbf", "h": h, "k": k, "thr": thr}, a.reshape(-1), L)
        for i, r in enumerate(a):
            pos, hv = oracle.nthash_seq(r.tobytes(), h, k)
            ev = np.zeros(L, np.uint8)
            eh = np.zeros(L, np.uint8)
            if len(pos):
                ev[pos.astype(np.int64)] = 1
                eh[pos.astype(np.int64)] = oracle.cbf_query(body, h, thr, hv)[1]
            assert (hit[i * L: (i + 1) * L] == eh).all() and (valid[i * L: (i + 1) * L] == ev).all(), (thr, i)
        res[thr] = hit
    assert (res[1] >= res[2]).all() and res[1].sum() > res[2].sum() > 0  # the threshold matters
    assert res[2][: (n // 2) * L].sum() == clean_windows(a[: n // 2].reshape(-1), L, k)  # inserted twice: all hit


def test_bitmap_bits_and_slice_ranges():
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, 1000).astype(np.uint8)
    words = np.zeros(16, np.uint64)
    for p in np.flatnonzero(bits):
        words[p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    for b0, b1 in ((0, 1000), (3, 64), (63, 65), (64, 128), (129, 997), (500, 500)):
        assert (bitmap_bits(words, b0, b1) == bits[b0:b1]).all(), (b0, b1)
    n = (1 << 20) + 77
    rs = slice_ranges(n, True)
    assert rs == [(0, 2048), (n - 2048, n), (65536 - 1024, 65536 + 1024), (15 * 65536 - 1024, 15 * 65536 + 1024)]
    assert slice_ranges(40000, False) == [(0, 2048), (37952, 40000), (18976, 21024)]
    assert slice_ranges(1500, False) == [(0, 1500), (0, 1500), (0, 1500)]
