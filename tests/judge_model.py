"""Plain host restatement of the three device-side judges (csrc/aux_kernels.hip: compare_kernel, popcount_kernel,
digest_kernel; include/btlbf.h: btlbf_compare, btlbf_popcount / btlbf_filtered_popcount / btlbf_popcount_bits,
btlbf_digest), in exact integers.

Dense forms take the local array as uint8 (bytes of a bit filter: bit p is bit p % 8 of byte p / 8; bytes of a counting
filter: one counter each).  Sparse forms take an otherwise empty array as a dict of its planted bytes
{byte offset in the local array: value 0..255}, so that arrays far too large for the host have an exactly known answer;
sparse_digest takes {index of the 64-bit word in the local array: value}, which words_of() makes from planted bytes."""
import numpy as np

M64 = (1 << 64) - 1

if hasattr(np, "bitwise_count"):
    def _bits_set(a):
        """number of set bits in a uint8 array"""
        n8 = a.size // 8 * 8
        return int(np.bitwise_count(a[:n8].view(np.uint64)).sum(dtype=np.uint64)) + int(np.bitwise_count(a[n8:]).sum())
else:
    _POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)

    def _bits_set(a):
        return int(np.bincount(a, minlength=256).astype(np.uint64) @ _POP8.astype(np.uint64))


def _u8(x):
    return np.ascontiguousarray(x, np.uint8).ravel()


def dense_compare(x, y, counting):
    """btlbf_compare(a, b): (positions that differ, positions with a > b, positions with a < b); positions are bits
    (a > b: set only in a) or uint8 counters"""
    x, y = _u8(x), _u8(y)
    assert x.size == y.size
    if counting:
        return int(np.count_nonzero(x != y)), int(np.count_nonzero(x > y)), int(np.count_nonzero(x < y))
    return _bits_set(x ^ y), _bits_set(x & ~y), _bits_set(y & ~x)


def dense_popcount(x, mode, thr=0):
    """popcount_kernel's modes over the local bytes -- 0: set bits, 1: non-zero bytes, 2: bytes >= thr (the padding an
    allocation adds is not part of the array: at thr == 0 every LOCAL byte counts, and no other)"""
    x = _u8(x)
    if mode == 0:
        return _bits_set(x)
    if mode == 1:
        return int(np.count_nonzero(x))
    if mode == 2:
        return int(np.count_nonzero(x >= thr)) if thr <= 255 else 0
    raise ValueError("mode %r" % (mode,))


def mix64(z):
    """the splitmix64 finaliser (include/btlbf.h, btlbf_digest)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sparse_digest(words, first_word=0):
    """btlbf_digest of an array whose non-zero 64-bit words are `words` = {index in the local array: value}: with
    i = first_word + index the word's index in the whole filter and m_i = mix64(i + 1) | 1,
    (sum of w_i * m_i mod 2^64, xor of mix64(w_i ^ m_i)); zero words contribute nothing"""
    s = x = 0
    for idx, w in words.items():
        w = int(w) & M64
        if not w:
            continue
        m = mix64((first_word + int(idx) + 1) & M64) | 1
        s = (s + w * m) & M64
        x ^= mix64(w ^ m)
    return s, x


def digest_with_word_replaced(digest, index, old, new, first_word=0):
    """the digest after the 64-bit word `index` of the local array changed from `old` to `new`: the digest is a sum and
    an xor over words, so one word's share can be taken out and put back"""
    so, xo = sparse_digest({index: old}, first_word)
    sn, xn = sparse_digest({index: new}, first_word)
    return (digest[0] - so + sn) & M64, digest[1] ^ xo ^ xn


def plant(planted, offset, data):
    """write the bytes `data` at byte `offset` into a planted-bytes dict; returns the dict"""
    for j, v in enumerate(bytes(data)):
        planted[offset + j] = v
    return planted


def words_of(planted):
    """{byte offset: value} -> {index of the little-endian 64-bit word: value}"""
    words = {}
    for off, v in planted.items():
        words[off >> 3] = words.get(off >> 3, 0) | (int(v) & 0xFF) << (8 * (off & 7))
    return words


def sparse_compare(a, b, counting):
    """dense_compare of two otherwise empty arrays given by their planted bytes"""
    differ = gt = lt = 0
    for off in set(a) | set(b):
        va, vb = int(a.get(off, 0)) & 0xFF, int(b.get(off, 0)) & 0xFF
        if counting:
            differ += va != vb
            gt += va > vb
            lt += va < vb
        else:
            differ += bin(va ^ vb).count("1")
            gt += bin(va & ~vb).count("1")
            lt += bin(vb & ~va).count("1")
    return differ, gt, lt


def sparse_popcount(a, mode, thr=0, local_bytes=None):
    """dense_popcount of an otherwise empty array of local_bytes bytes given by its planted bytes (local_bytes is
    needed only where zero bytes count: mode 2 at thr == 0)"""
    vals = [int(v) & 0xFF for v in a.values()]
    if mode == 0:
        return sum(bin(v).count("1") for v in vals)
    if mode == 1:
        return sum(v != 0 for v in vals)
    if mode == 2:
        if thr == 0:
            return int(local_bytes)
        return sum(v >= thr for v in vals)
    raise ValueError("mode %r" % (mode,))


def sparse_to_dense(planted, nbytes):
    out = np.zeros(nbytes, np.uint8)
    for off, v in planted.items():
        out[off] = v
    return out
