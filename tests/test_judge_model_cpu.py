"""tests/judge_model.py against itself and against engine.body_digest, on the host: the model the GPU judge tests
(test_gpu_judges.py) take their exact expectations from must itself be pinned -- the dense forms to a brute-force
unpackbits / elementwise restatement, sparse_digest to body_digest, the sparse forms to the dense ones."""
import numpy as np
import pytest

import judge_model as jm

SIZES = [8, 125, 4096, 100_001]  # 125 and 100 001: the last 64-bit word is padded


def _body(rng, n):
    """random bytes with zero runs and every counter value the thresholds of the GPU tests ask about"""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    runs = np.repeat(rng.random((n + 63) // 64) < 0.4, 64)[:n]
    b[runs] = 0
    b[rng.integers(0, n, max(1, n // 50))] = rng.choice(np.array([0, 1, 2, 200, 255], np.uint8), max(1, n // 50))
    return b


def _pair(n):
    rng = np.random.default_rng(n)
    x = _body(rng, n)
    y = x.copy()
    idx = np.unique(rng.integers(0, n, min(1000, max(1, n // 3))))
    y[idx] = rng.integers(0, 256, idx.size, dtype=np.uint8)
    return x, y


def _words(body):
    b = np.concatenate([body, np.zeros(-body.size % 8, np.uint8)])
    return {i: int(w) for i, w in enumerate(b.view("<u8").tolist())}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("first_word", [0, 3, (1 << 33) + 5])
def test_sparse_digest_equals_body_digest(n, first_word):
    from btl_bloomfilter_amd.engine import body_digest

    x, y = _pair(n)
    for body in (x, y):
        assert jm.sparse_digest(_words(body), first_word) == body_digest(body, first_word=first_word) != (0, 0)
    assert jm.sparse_digest({}) == (0, 0) == jm.sparse_digest({5: 0, 9: 0})
    # position dependent: the same word elsewhere gives another digest
    assert jm.sparse_digest({0: 1}) != jm.sparse_digest({1: 1}) != jm.sparse_digest({0: 1}, first_word=2)


@pytest.mark.parametrize("n", SIZES)
def test_digest_with_word_replaced_equals_body_digest_of_the_changed_body(n):
    from btl_bloomfilter_amd.engine import body_digest

    x, _ = _pair(n)
    d = body_digest(x, first_word=7)
    for off in (0, n // 2, n - 1):
        for new in (x[off] ^ 0x10, 0, 255):
            z = x.copy()
            z[off] = new
            old_w, new_w = _words(x)[off >> 3], _words(z)[off >> 3]
            assert jm.digest_with_word_replaced(d, off >> 3, old_w, new_w, first_word=7) == body_digest(z, first_word=7)


@pytest.mark.parametrize("n", SIZES)
def test_dense_compare_equals_brute_force(n):
    x, y = _pair(n)
    bx, by = np.unpackbits(x), np.unpackbits(y)
    want = int((bx != by).sum()), int((bx > by).sum()), int((bx < by).sum())
    assert jm.dense_compare(x, y, False) == want
    assert jm.dense_compare(y, x, False) == (want[0], want[2], want[1])
    assert want[0] == want[1] + want[2]
    if n >= 4096:
        assert want[1] > 0 and want[2] > 0
    xi, yi = x.astype(int).tolist(), y.astype(int).tolist()
    wantc = sum(a != b for a, b in zip(xi, yi)), sum(a > b for a, b in zip(xi, yi)), sum(a < b for a, b in zip(xi, yi))
    assert jm.dense_compare(x, y, True) == wantc
    assert jm.dense_compare(y, x, True) == (wantc[0], wantc[2], wantc[1])
    assert jm.dense_compare(x, x, False) == (0, 0, 0) == jm.dense_compare(x, x, True)


@pytest.mark.parametrize("n", SIZES)
def test_dense_popcount_equals_brute_force(n):
    x, _ = _pair(n)
    xi = x.astype(int).tolist()
    assert jm.dense_popcount(x, 0) == int(np.unpackbits(x).sum()) == sum(bin(v).count("1") for v in xi)
    assert jm.dense_popcount(x, 1) == sum(v != 0 for v in xi)
    for thr in (0, 1, 2, 200, 255, 256):
        assert jm.dense_popcount(x, 2, thr) == sum(v >= thr for v in xi)
    assert jm.dense_popcount(x, 2, 0) == n  # every local byte, and no padding
    if n >= 4096:
        assert jm.dense_popcount(x, 2, 1) > jm.dense_popcount(x, 2, 2) > jm.dense_popcount(x, 2, 200) > jm.dense_popcount(x, 2, 255) > 0


@pytest.mark.parametrize("n", SIZES)
def test_sparse_forms_equal_dense_forms_on_the_same_planted_bytes(n):
    from btl_bloomfilter_amd.engine import body_digest

    rng = np.random.default_rng(n + 1)
    a, b = {}, {}
    offs = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 40)])).tolist()
    for i, off in enumerate(offs):
        va, vb = (int(v) for v in rng.integers(1, 256, 2))
        if i % 4 == 0:
            a[off] = b[off] = va        # shared, equal
        elif i % 4 == 1:
            a[off], b[off] = va, vb     # shared word, other value
        elif i % 4 == 2:
            a[off] = va
        else:
            b[off] = vb
    a[offs[1]] = 0  # a planted zero byte is an empty position
    jm.plant(a, min(n - 8, 16) if n > 8 else 0, (0x0123456789ABCDEF).to_bytes(8, "little"))
    da, db = jm.sparse_to_dense(a, n), jm.sparse_to_dense(b, n)
    for counting in (False, True):
        assert jm.sparse_compare(a, b, counting) == jm.dense_compare(da, db, counting)
        assert jm.sparse_compare(b, a, counting) == jm.dense_compare(db, da, counting)
        assert jm.sparse_compare(a, a, counting) == (0, 0, 0)
    for planted, dense in ((a, da), (b, db)):
        assert jm.sparse_popcount(planted, 0) == jm.dense_popcount(dense, 0)
        assert jm.sparse_popcount(planted, 1) == jm.dense_popcount(dense, 1)
        for thr in (0, 1, 2, 200, 255):
            assert jm.sparse_popcount(planted, 2, thr, local_bytes=n) == jm.dense_popcount(dense, 2, thr)
        for fw in (0, 1 << 30):
            assert jm.sparse_digest(jm.words_of(planted), fw) == body_digest(dense, first_word=fw)
