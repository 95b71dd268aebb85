"""numpy restatement of the reference's multi-index Bloom filter (miBF) stages 3-4, the checker of tests/test_gpu_mibf.py
and tests/test_mibf_cpu.py.  Written from the reference's text (MIBloomFilter.hpp, MIBFConstructSupport.hpp,
MIBFQuerySupport.hpp) and pinned to the reference's own build by tests/test_mibf_vs_ref.py (oracle/ref_mibf_driver.cpp).
rank() is a cumulative sum over the stage-1 bit vector and the dense_hash_set walk is the ascending order this library
documents (include/btlbf.h).
Inputs are hash rows as btlbf_hash_seqs emits them (hash_seqs / sthash_seqs): window p of the buffer at row p, valid
bit p set iff the iterator emits the window."""
import struct

import numpy as np

VERSION = 1  # MIBloomFilter_VERSION


def masks(id_bytes):
    """s_mask = 1 << (bits(T)-1), s_antiMask = ~s_mask (MIBloomFilter.hpp:36-37)"""
    bits = 8 * id_bytes
    return 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << bits) - 1


class Ranks:
    """getRankPos(hash) = rank(hash % size) (MIBloomFilter.hpp:527) over the stage-1 bit vector (filter body bytes,
    bit p = bit p%8 of byte p/8); bit(hash) = m_bv[hash % size] (atRank, :478-515)"""

    def __init__(self, body, size):
        self.size = int(size)
        self.bits = np.unpackbits(np.asarray(body, np.uint8), bitorder="little")[: self.size]
        self.csum = np.concatenate([[0], np.cumsum(self.bits, dtype=np.uint64)])
        self.pop = int(self.csum[-1])

    def pos(self, hv):
        return (np.asarray(hv, np.uint64) % np.uint64(self.size)).astype(np.int64)

    def rank(self, hv):
        return self.csum[self.pos(hv)].astype(np.int64)

    def bit(self, hv):
        return self.bits[self.pos(hv)].astype(bool)


def window_seqs(n_bytes, starts=None, read_len=0):
    """sequence index of every window start offset of a buffer"""
    if read_len:
        return np.arange(n_bytes, dtype=np.int64) // read_len
    st = np.asarray(starts, np.int64)
    return np.searchsorted(st, np.arange(n_bytes), side="right") - 1


def set_data(old, new_id, id_bytes):
    """setData (MIBloomFilter.hpp:625-634): the id keeps the saturation bit iff the old value is > mask"""
    mask, _, _ = masks(id_bytes)
    return (new_id | mask) if old > mask else new_id


def insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes):
    """insertMIBF (MIBFConstructSupport.hpp:109-130) of every sequence in order, in place on data / counts (int64 numpy
    arrays of pop entries holding T values).  V = distinct hash values of the sequence's clean windows, walked in
    ascending order; count = T(count + 1); replace when count != 0 and T(v ^ id) % count == count - 1."""
    _, _, full = masks(id_bytes)
    rows = np.asarray(rows, np.uint64)
    v = rows[valid].ravel()
    s = np.repeat(wseq[valid], rows.shape[1])
    order = np.lexsort((v, s))  # by sequence, then value
    v, s = v[order], s[order]
    keep = np.ones(v.size, bool)
    keep[1:] = (v[1:] != v[:-1]) | (s[1:] != s[:-1])
    v, s = v[keep], s[keep]
    r = ranks.rank(v)
    o = np.argsort(r, kind="stable")  # events of one rank in (sequence, value) order
    v, s, r = v[o], s[o], r[o]
    if r.size == 0:
        return
    head = np.ones(r.size, bool)
    head[1:] = r[1:] != r[:-1]
    gstart = np.maximum.accumulate(np.where(head, np.arange(r.size), 0))
    j = np.arange(r.size) - gstart
    idv = np.asarray(ids, np.int64)[s] & full
    c = (counts[r] + j + 1) & full
    x = ((v & np.uint64(full)).astype(np.int64) ^ idv) & full
    rep = (c != 0) & (x % np.where(c == 0, 1, c) == c - 1)
    ur, first = np.unique(r, return_index=True)
    glen = np.diff(np.concatenate([first, [r.size]]))
    counts[ur] = (counts[ur] + glen) & full
    for e in np.nonzero(rep)[0]:  # in order: setData's chain per rank
        data[r[e]] = set_data(int(data[r[e]]), int(idv[e]), id_bytes)


def _decide(rk, x, idv, counts, h):
    """setSatIfMissing's choice for one window (MIBFConstructSupport.hpp:166-213): None = found, -1 = saturate,
    else the position to mutate.  seenSet and replacementIDs both start with h zeros."""
    seen = [0] * h
    repl = [0] * h
    for i in range(h):
        if x[i] == idv:
            return None
        if x[i] not in seen:
            seen.append(x[i])
        else:
            repl.append(x[i])
    pos, min_count = -1, 0  # numeric_limits<T>::min()
    for i in range(h):
        if x[i] in repl and min_count < counts[rk[i]]:
            min_count = counts[rk[i]]
            pos = rk[i]
    return pos


def saturate_serial(data, counts, ranks, rows, valid, wseq, ids, id_bytes):
    """insertSaturation in the reference's single-threaded order (BTLBF_ORDER_SERIAL) -> [clean, found, mutated,
    saturated]"""
    mask, anti, full = masks(id_bytes)
    rows = np.asarray(rows, np.uint64)
    h = rows.shape[1]
    out = [0, 0, 0, 0]
    for p in np.nonzero(valid)[0]:
        out[0] += 1
        idv = int(ids[wseq[p]]) & full
        rk = [int(q) for q in ranks.rank(rows[p])]
        x = [int(data[q]) & anti for q in rk]
        pos = _decide(rk, x, idv, counts, h)
        if pos is None:
            out[1] += 1
        elif pos >= 0:
            out[2] += 1
            data[pos] = set_data(int(data[pos]), idv, id_bytes)
            counts[pos] = (int(counts[pos]) + 1) & full
        else:
            out[3] += 1
            for q in rk:  # saturate(hashes), MIBloomFilter.hpp:440-446
                data[q] = int(data[q]) | mask
    return out


def saturate_parallel(data, counts, ranks, rows, valid, wseq, ids, id_bytes):
    """BTLBF_ORDER_PARALLEL: every window decides against the arrays as they stood at the start of the call; each
    mutated position gets counts += its choosers and the id of its last chooser (setData against the start value);
    then every saturation is ORed in -> [clean, found, mutated, saturated]"""
    mask, anti, full = masks(id_bytes)
    rows = np.asarray(rows, np.uint64)
    h = rows.shape[1]
    d0, c0 = data.copy(), counts.copy()
    out = [0, 0, 0, 0]
    choosers, last, sat = {}, {}, []
    for p in np.nonzero(valid)[0]:
        out[0] += 1
        idv = int(ids[wseq[p]]) & full
        rk = [int(q) for q in ranks.rank(rows[p])]
        x = [int(d0[q]) & anti for q in rk]
        pos = _decide(rk, x, idv, c0, h)
        if pos is None:
            out[1] += 1
        elif pos >= 0:
            out[2] += 1
            choosers[pos] = choosers.get(pos, 0) + 1
            last[pos] = idv
        else:
            out[3] += 1
            sat.extend(rk)
    for pos, n in choosers.items():
        counts[pos] = (int(c0[pos]) + n) & full
        data[pos] = set_data(int(d0[pos]), last[pos], id_bytes)
    for q in sat:
        data[q] = int(data[q]) | mask
    return out


def query(data, ranks, rows, valid, max_miss, spaced):
    """getMatchSignature (MIBFQuerySupport.hpp:158-217) over atRank (MIBloomFilter.hpp:478-515) -> (values[n, h] raw T
    values, match bool[n]).  Seeds: at most max_miss clear bits; no seeds: all h bits."""
    rows = np.asarray(rows, np.uint64)
    n, h = rows.shape
    bit = ranks.bit(rows.ravel()).reshape(n, h)
    rk = ranks.rank(rows.ravel()).reshape(n, h)
    misses = h - bit.sum(axis=1)
    match = valid & ((misses <= max_miss) if spaced else (misses == 0))
    vals = np.where(match[:, None] & bit, np.asarray(data, np.int64)[np.minimum(rk, max(len(data) - 1, 0))], 0)
    return vals, match


def stats(data, id_bytes):
    """getPopNonZero, getPopSaturated (strict > mask) (MIBloomFilter.hpp:580-620)"""
    mask, _, _ = masks(id_bytes)
    d = np.asarray(data, np.int64)
    return int((d != 0).sum()), int((d > mask).sum())


def id_counts(data, n_ids, id_bytes):
    """getIDCounts (MIBloomFilter.hpp:539-551); ids >= n_ids are not counted"""
    mask, anti, _ = masks(id_bytes)
    d = np.asarray(data, np.int64)
    b = np.where(d > mask, d & anti, d)
    return np.bincount(b[b < n_ids], minlength=n_ids).astype(np.uint64), int((d > mask).sum())


def header(size, nhash, kmer, seeds=()):
    """the packed FileHeader (MIBloomFilter.hpp:106-117) as writeHeader fills it (:722-742), then the seeds"""
    hlen = 32 + kmer * len(seeds)
    return struct.pack("<8sIQIII", b"MIBLOOMF", hlen, size, nhash, kmer, VERSION) + b"".join(
        s.encode() if isinstance(s, str) else s for s in seeds)


def file_bytes(data, id_bytes, nhash, kmer, seeds=()):
    dt = np.dtype("<u2") if id_bytes == 2 else np.dtype("<u4")
    return header(len(data), nhash, kmer, seeds) + np.asarray(data).astype(dt).tobytes()
