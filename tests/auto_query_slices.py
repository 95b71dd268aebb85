"""CPU side of the AUTO-query tests (test_gpu_auto_query.py): the expected contains() bits of slices of whole
fixed-length reads, computed by the CPU oracle from a downloaded filter body -- independent of both GPU paths --, and
the small bitmap / window arithmetic the tests share.  Plain functions, tested on the CPU by
test_auto_query_slices_cpu.py."""
import numpy as np

BASES = np.frombuffer(b"ACGTacgt", np.uint8)


def expected_slice_bits(oracle, body, params, reads, L):
    """Expected (hit, valid) of a buffer of whole reads of L bytes, one uint8 (0 / 1) per BYTE of `reads`.

    body:   the filter's downloaded array (bits, or uint8 counters)
    params: {"kind": "bf", "bits": ..., "h": ..., "k": ...} or {"kind": "cbf", "h": ..., "k": ..., "thr": ...}
    reads:  uint8 array, a whole number of reads

    The oracle sees the slice as ONE sequence, so it also answers for the windows that straddle two reads; those --
    every window that starts at an offset > L - k inside its read -- are not windows of the fixed-length layout and
    are set to 0 in both arrays, which is what the GPU bitmaps must hold there."""
    reads = np.ascontiguousarray(reads, np.uint8).reshape(-1)
    n_bytes, k, h = reads.size, params["k"], params["h"]
    assert L >= k and n_bytes % L == 0
    hit = np.zeros(n_bytes, np.uint8)
    valid = np.zeros(n_bytes, np.uint8)
    if n_bytes == 0:
        return hit, valid
    seq = reads.tobytes()
    if params["kind"] == "bf":
        eh, ev = oracle.bf_contains_seq_dense(body, params["bits"], h, k, seq)
        hit[: eh.size] = eh
        valid[: ev.size] = ev
    else:
        pos, hv = oracle.nthash_seq(seq, h, k)  # the clean windows and their hash rows
        if pos.size:
            _, ct = oracle.cbf_query(body, h, params["thr"], hv)
            p = pos.astype(np.int64)
            valid[p] = 1
            hit[p] = ct
    keep = np.arange(L) <= L - k
    hit = (hit.reshape(-1, L) * keep).reshape(-1).astype(np.uint8)
    valid = (valid.reshape(-1, L) * keep).reshape(-1).astype(np.uint8)
    return hit, valid


def bitmap_bits(words, b0, b1):
    """bits [b0, b1) of a bitmap of 64-bit words (bit p & 63 of word p >> 6) as uint8 0 / 1"""
    by = np.ascontiguousarray(words).view(np.uint8)
    lo, hi = b0 // 8, (b1 + 7) // 8
    return np.unpackbits(by[lo:hi], bitorder="little")[b0 - 8 * lo: b1 - 8 * lo]


def clean_windows(reads, L, k):
    """clean windows (all k bytes in ACGTacgt, start offset <= L - k) of a buffer of whole reads"""
    a = np.ascontiguousarray(reads, np.uint8).reshape(-1, L)
    W = L - k + 1
    is_base = np.zeros(256, bool)
    is_base[BASES] = True
    rows = np.flatnonzero(~is_base[a].all(axis=1))  # only these reads have an unclean window
    total = (a.shape[0] - rows.size) * W
    if rows.size:
        bad = np.zeros((rows.size, L + 1), np.int64)
        bad[:, 1:] = np.cumsum(~is_base[a[rows]], axis=1)
        total += int((bad[:, k:] - bad[:, :W] == 0).sum())
    return total


def slice_ranges(n_reads, large):
    """[r0, r1) read ranges the oracle checks: both ends of the buffer (the last one with the ragged tail of the last
    flag word), 1024 reads either side of read 65536 -- where the second 1024-word chunk of the flag array starts --
    or, for a buffer that does not reach it, either side of the middle; `large`: also either side of read 15 x 65536"""
    edge = min(2048, n_reads)
    rs = [(0, edge), (n_reads - edge, n_reads)]
    mids = [65536 if n_reads > 65536 + 1024 else n_reads // 2] + ([15 * 65536] if large else [])
    for m in mids:
        rs.append((max(m - 1024, 0), min(m + 1024, n_reads)))
    assert sum(b - a for a, b in rs) <= 1 << 14
    return rs
