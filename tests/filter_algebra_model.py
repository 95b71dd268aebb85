"""TEST-ONLY: the filter algebra (btlbf_combine / btlbf_fold / btlbf_threshold_bits) restated with numpy over host copies
of filter bodies, in exact integers.  A body is a uint8 array; `counter_bytes` is 0 for a bit filter, else the counter's
width.  tests/test_filter_algebra_model_cpu.py pins this model to filters built by the oracle; the GPU tests then use it."""
import numpy as np

OR, AND, ANDNOT, ADD, MAX, MIN = range(6)
BIT_OPS, COUNTER_OPS = (OR, AND, ANDNOT), (ADD, MAX, MIN)


def _view(body, counter_bytes):
    b = np.ascontiguousarray(body, np.uint8)
    return b.view("<u%d" % counter_bytes) if counter_bytes else b


def counter_max(counter_bytes):
    return (1 << (8 * counter_bytes)) - 1


def combine(dst, srcs, op, counter_bytes):
    """(body of dst OP srcs[0] OP ..., its popcount: set bits / non-zero counters)"""
    d = _view(dst, counter_bytes).copy()
    if counter_bytes == 0:
        assert op in BIT_OPS
        for s in srcs:
            s = _view(s, 0)
            d = d | s if op == OR else d & s if op == AND else d & ~s
        return d, int(np.unpackbits(d).sum())
    assert op in COUNTER_OPS
    mx = counter_max(counter_bytes)
    acc = [int(x) for x in d]  # exact: python integers
    for s in srcs:
        sv = [int(x) for x in _view(s, counter_bytes)]
        if op == ADD:
            acc = [min(a + b, mx) for a, b in zip(acc, sv)]
        elif op == MAX:
            acc = [max(a, b) for a, b in zip(acc, sv)]
        else:
            acc = [min(a, b) for a, b in zip(acc, sv)]
    out = np.array(acc, dtype="<u%d" % counter_bytes)
    return out.view(np.uint8), int(np.count_nonzero(out))


def combine_fast(dst, srcs, op, counter_bytes):
    """combine() for large bodies: the same arithmetic in numpy's own integers (ADD through a float-free widening: the sum
    of two saturating operands is computed as a + min(b, MAX - a))"""
    if counter_bytes == 0:
        return combine(dst, srcs, op, 0)
    d = _view(dst, counter_bytes).copy()
    mx = d.dtype.type(counter_max(counter_bytes))
    for s in srcs:
        s = _view(s, counter_bytes)
        d = d + np.minimum(s, mx - d) if op == ADD else np.maximum(d, s) if op == MAX else np.minimum(d, s)
    return d.view(np.uint8), int(np.count_nonzero(d))


def fold(body, factor, counter_bytes):
    """the body of size / factor positions: position p combines source positions p + j * size / factor (OR; saturating
    ADD).  For a bit filter the slices are whole bytes (size / factor is a multiple of 8)."""
    b = _view(body, counter_bytes)
    assert b.size % factor == 0
    rows = b.reshape(factor, b.size // factor)
    if counter_bytes == 0:
        return np.bitwise_or.reduce(rows, axis=0)
    mx = counter_max(counter_bytes)
    if counter_bytes < 8:
        assert factor * mx < 1 << 64  # the exact sum fits 64 bits
        out = np.minimum(rows.sum(axis=0, dtype=np.uint64), np.uint64(mx))
        return out.astype("<u%d" % counter_bytes).view(np.uint8)
    acc = np.zeros(rows.shape[1], np.uint64)
    for r in rows:  # 64-bit counters: saturate step by step
        acc = acc + np.minimum(r, np.uint64(mx) - acc)
    return acc.view(np.uint8)


def threshold_bits(body, threshold, counter_bytes):
    """the bit filter body with bit p = (counter p >= threshold); the counter count is a multiple of 8"""
    c = _view(body, counter_bytes)
    assert counter_bytes and c.size % 8 == 0
    if threshold > counter_max(counter_bytes):
        return np.zeros(c.size // 8, np.uint8)
    return np.packbits(c >= c.dtype.type(threshold), bitorder="little")
