"""What the read-modify-write operations may produce in PARALLEL order, as plain numpy checkers, and a CPU
interleaving simulator that is the evidence for them.  No GPU import: tests/test_update_order_cpu.py runs the
simulator against the checkers, tests/test_gpu_update_order.py runs the HIP kernels against the same checkers.

The operations are the four whose result depends on who gets there first: BloomFilter::insertAndCheck
(BloomFilter.hpp:200-214, one fetch-or per probe) and CountingBloomFilter::incrementAll / incrementMin /
insertAndCheck (CountingBloomFilter.hpp:135-183,206-214: byte loads and byte compare-and-swaps).  Every property
below holds for EVERY interleaving of those per-probe atomics -- the argument is next to each -- so a kernel that
violates one is wrong, whatever order its lanes ran in.

Conventions: a filter body is the uint8 array download() returns; `pos` is an (n, h) integer array of probe
positions, row = one clean window, `hashes % size` of the oracle's hash rows (positions()); a checker raises
ContractViolation (an AssertionError) whose `.prop` names the property and whose text names the first offending
counter, bit or window.
"""
import random

import numpy as np


class ContractViolation(AssertionError):
    def __init__(self, prop, msg):
        super().__init__("%s: %s" % (prop, msg))
        self.prop = prop


def _require(ok, prop, msg, *args):
    if not ok:
        raise ContractViolation(prop, msg % args)


def _none(bad, prop, fmt, *cols):
    """no element of `bad` may be set; the message gets the first offender's index and its entry of every column"""
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ContractViolation(prop, fmt % ((i,) + tuple(c[i] if np.ndim(c) else c for c in cols)))


def positions(hashes, size):
    """(n, h) uint64 hash rows -> (n, h) int64 positions, the reference's `hash % m_size`"""
    hv = np.ascontiguousarray(hashes, np.uint64)
    return (hv % np.uint64(size)).astype(np.int64)


def unpack_bits(body, size_bits):
    """bit p = bit p % 8 of byte p / 8 (BloomFilter.hpp:190-192) -> bool[size_bits]"""
    return np.unpackbits(np.ascontiguousarray(body, np.uint8), bitorder="little")[:size_bits].astype(bool)


def _windows_per_position(pos, size):
    """how many distinct windows probe each position"""
    n, h = pos.shape
    key = np.unique(np.arange(n, dtype=np.int64).repeat(h) * size + pos.ravel())
    return np.bincount(key % size, minlength=size)


# ---------------------------------------------------------------------------------------------------------------
# bit filter: insertAndCheck
# ---------------------------------------------------------------------------------------------------------------
def check_bit_insert_and_check(size_bits, before, after, expect_after, pos, out):
    """P1-P5.  `expect_after`: oracle.bf_insert of the same windows on a copy of `before`; `out`: the report of
    every window of `pos` (1 = all h bits were found set)."""
    out = np.asarray(out).astype(np.uint8)
    pos = np.asarray(pos, np.int64).reshape(len(out), -1)
    h = pos.shape[1]
    after, expect_after = np.asarray(after), np.asarray(expect_after)
    b, a = unpack_bits(before, size_bits), unpack_bits(after, size_bits)
    # P1: fetch-or is an OR whatever it returns: the bits are those of insert()
    _none(after != expect_after, "P1", "body byte %d is 0x%02x, insert() of the same windows gives 0x%02x", after,
          expect_after)
    _none(out > 1, "P2", "window %d reports %d, not 0 or 1", out)
    if len(out) == 0:
        return
    # P2: bits are never cleared, so every fetch-or of such a window returns 1
    _none(b[pos].all(axis=1) & (out != 1), "P2", "window %d reports 0 although its %d bits were all set before the call", h)
    # P3: the fetch-or that set a bit returned 0 to its window
    new = a & ~b
    by_zero = np.zeros(size_bits, bool)
    by_zero[pos[out == 0].ravel()] = True
    _none(new & ~by_zero, "P3", "bit %d was newly set, yet no window that probes it reports 0")
    # P4: that window's own first fetch-or of the bit is the one that set it
    alone = _windows_per_position(pos, size_bits) == 1
    _none((~b[pos] & alone[pos]).any(axis=1) & (out != 0), "P4",
          "window %d reports 1 although it alone probes a bit that was clear")
    # P5: a window that reports 0 was the first to set some bit, and a bit has one first setter
    zeros, n_new = int((out == 0).sum()), int(new.sum())
    _require(zeros <= n_new, "P5", "%d windows report 0 but only %d bits were newly set", zeros, n_new)
    if h == 1:
        _require(zeros == n_new, "P5", "h = 1: %d windows report 0 for %d newly set bits", zeros, n_new)


def check_window_bitmaps(hit_bits, valid_bits, counts, n_bytes, clean_pos):
    """P6 of the sequence form: valid bitmap == the oracle's clean windows (`clean_pos`, byte offsets into the
    buffer), hit bits 0 outside it, counts == [clean, popcount(hit)].  -> the report of every clean window, in
    `clean_pos` order, for check_bit_insert_and_check."""
    def unpack(words):
        return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)

    hit, valid = unpack(hit_bits), unpack(valid_bits)
    _require(hit.size == valid.size == (n_bytes + 63) // 64 * 64, "P6", "bitmaps of %d and %d bits for %d bytes", hit.size,
             valid.size, n_bytes)
    clean_pos = np.asarray(clean_pos, np.int64)
    exp = np.zeros(valid.size, bool)
    exp[clean_pos] = True
    _none(valid != exp, "P6", "valid bit of window %d is %d, the oracle says %d", valid, exp)
    _none(hit & ~exp, "P6", "hit bit set at window %d, which is not clean")
    if counts is not None:
        got = [int(x) for x in np.asarray(counts).ravel()[:2]]
        _require(got == [int(exp.sum()), int(hit.sum())], "P6", "counts %s, expected [clean %d, hits %d]", got,
                 int(exp.sum()), int(hit.sum()))
    return hit[clean_pos].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# counting filter
# ---------------------------------------------------------------------------------------------------------------
def check_increment_all(after, expect_after):
    """A1: saturating +1 commutes -- the counters are oracle.cbf_increment_all's, exactly"""
    after, expect_after = np.asarray(after), np.asarray(expect_after)
    _require(after.shape == expect_after.shape, "A1", "body of %d counters, expected %d", after.size, expect_after.size)
    _none(after != expect_after, "A1", "counter %d is %d, incrementAll gives %d", after, expect_after)


def check_increment_min(before, after, upper, pos):
    """M1-M4.  `upper`: oracle.cbf_increment_all of the same windows on a copy of `before`."""
    before, after, upper = (np.asarray(x, np.uint8).astype(np.int64) for x in (before, after, upper))
    pos = np.asarray(pos, np.int64)
    size = before.size
    _require(after.size == size, "M1", "body of %d counters, expected %d", after.size, size)
    touched = np.zeros(size, bool)
    touched[pos.ravel()] = True
    # M1: the only write is a compare-and-swap v -> v + 1 with v < 255, on a counter of the window
    _none(after < before, "M1", "counter %d decreased from %d to %d", before, after)
    _none((before == 255) & (after != 255), "M1", "counter %d was 255 and is %d", after)
    _none(~touched & (after != before), "M1", "counter %d is probed by no window and went from %d to %d", before, after)
    # M2: one incrementMin raises each of its counters at most once (after its compare-and-swap m -> m + 1 the
    # counter is above m for good); incrementAll raises it once per probe
    _none(after > upper, "M2", "counter %d is %d, above incrementAll's %d", after, upper)
    if pos.size == 0:
        return
    # M3: a window leaves its loop after a pass over its counters with the minimum m >= min(before) it read: every
    # counter still at m was raised by that pass, every other one was above m already
    need = np.minimum(before[pos].min(axis=1) + 1, 255)
    got = after[pos].min(axis=1)
    _none(got < need, "M3", "window %d: minimum %d after the call, at least %d required (minimum before + 1, or 255)", got,
          need)
    # M4: without saturation every window's loop ends with at least one and at most h successful swaps
    if upper[touched].max() < 255:
        n, h = pos.shape
        grew = int(after.sum() - before.sum())
        _require(n <= grew <= h * n, "M4", "the counters grew by %d in all; %d windows of %d probes allow %d .. %d", grew,
                 n, h, n, h * n)


def check_counting_insert_and_check(before, after, upper, pos, out, thr):
    """insertAndCheck = contains() then incrementMin (CountingBloomFilter.hpp:206-214): counters only grow and stay
    below `upper` (M2), so a minimum >= thr before the call is one at any time (C1) and a minimum < thr in `upper` is
    one at any time (C0); the body obeys M1-M4."""
    b, u = np.asarray(before, np.uint8).astype(np.int64), np.asarray(upper, np.uint8).astype(np.int64)
    pos = np.asarray(pos, np.int64)
    out = np.asarray(out).astype(np.uint8)
    _require(len(out) == len(pos), "C1", "%d reports for %d windows", len(out), len(pos))
    if len(out):
        _none((b[pos].min(axis=1) >= thr) & (out != 1), "C1",
              "window %d reports %d although its minimum was >= %d before the call", out, thr)
        _none((u[pos].min(axis=1) < thr) & (out != 0), "C0",
              "window %d reports %d although even incrementAll leaves its minimum < %d", out, thr)
    check_increment_min(before, after, upper, pos)


# ---------------------------------------------------------------------------------------------------------------
# the interleaving simulator.  A window is a generator that performs exactly ONE atomic memory operation per
# step (the code up to its next `yield`); a seeded scheduler interleaves the steps of the windows in flight.
# `mem` is a list of ints: bits for the bit filter, uint8 counters for the counting filter.
# ---------------------------------------------------------------------------------------------------------------
def simulate(op, mem, rows, seed, in_flight=64, **kw):
    """run op(mem, row, **kw) for every row with at most `in_flight` windows started and unfinished at a time
    (they start in row order, as lanes take their windows); -> the windows' return values"""
    rng = random.Random(seed)
    rows = [[int(p) for p in r] for r in rows]
    results = [None] * len(rows)
    live, nxt = [], 0
    while live or nxt < len(rows):
        while len(live) < in_flight and nxt < len(rows):
            live.append((nxt, op(mem, rows[nxt], **kw)))
            nxt += 1
        j = rng.randrange(len(live))
        try:
            next(live[j][1])
        except StopIteration as e:
            results[live[j][0]] = e.value
            live[j] = live[-1]
            live.pop()
    return results


# -- the reference, step by step ----------------------------------------------------------------------------------
def ref_bit_insert_and_check(mem, row):
    found = 1
    for p in row:
        old, mem[p] = mem[p], 1  # __sync_fetch_and_or
        found &= old
        yield
    return found


def ref_increment_all(mem, row):
    for p in row:
        while True:
            cur = mem[p]  # currentVal = m_filter[pos]
            yield
            if cur == 255:  # newVal < currentVal
                break
            ok = mem[p] == cur  # __sync_bool_compare_and_swap
            if ok:
                mem[p] = cur + 1
            yield
            if ok:
                break


def _ref_min_count(mem, row):
    mn = 255
    for p in row:
        mn = min(mn, mem[p])
        yield
    return mn


def ref_increment_min(mem, row):
    mn = yield from _ref_min_count(mem, row)
    done = False
    while not done:
        if mn == 255:  # minVal > newVal
            return
        for p in row:
            if mem[p] == mn:  # __sync_bool_compare_and_swap(minVal, newVal)
                mem[p] = mn + 1
                done = True
            yield
        if not done:
            mn = yield from _ref_min_count(mem, row)


def ref_counting_insert_and_check(mem, row, thr=1):
    found = int((yield from _ref_min_count(mem, row)) >= thr)
    yield from ref_increment_min(mem, row)
    return found


# -- the same on 32-bit words of four counters, as a device without byte atomics has to do it -----------------------
def _wload(mem, w):
    return mem[4 * w] | mem[4 * w + 1] << 8 | mem[4 * w + 2] << 16 | mem[4 * w + 3] << 24


def _wstore(mem, w, v):
    for i in range(4):
        mem[4 * w + i] = (v >> (8 * i)) & 0xff


def _wcas(mem, w, old, new):
    cur = _wload(mem, w)
    if cur == old:
        _wstore(mem, w, new)
    return cur


def _word_cas_byte(mem, p, expect):
    """byte compare-and-swap expect -> expect + 1 through a word compare-and-swap: a failure that only a neighbour
    caused is retried for as long as the own byte still holds `expect`"""
    w, sh = p >> 2, (p & 3) * 8
    old = _wload(mem, w)
    yield
    while True:
        if (old >> sh) & 0xff != expect:
            return False
        prev = _wcas(mem, w, old, old + (1 << sh))
        yield
        if prev == old:
            return True
        old = prev


def _word_min_count(mem, row):
    mn = 255
    for p in row:
        mn = min(mn, (_wload(mem, p >> 2) >> ((p & 3) * 8)) & 0xff)
        yield
    return mn


def word_increment_min(mem, row):
    """incrementMin with word compare-and-swaps, done right (the positive control of the two mutants below)"""
    while True:
        mn = yield from _word_min_count(mem, row)
        if mn == 255:
            return
        done = False
        for p in row:
            done |= yield from _word_cas_byte(mem, p, mn)
        if done:
            return


def word_increment_all(mem, row):
    """incrementAll with word compare-and-swaps, done right (the positive control of mutant_all_no_saturation_test)"""
    for p in row:
        w, sh = p >> 2, (p & 3) * 8
        old = _wload(mem, w)
        yield
        while (old >> sh) & 0xff != 255:
            prev = _wcas(mem, w, old, old + (1 << sh))
            yield
            if prev == old:
                break
            old = prev


# -- mutants: each is one of the above with one plausible mistake ------------------------------------------------------
def mutant_all_lost_update(mem, row):
    """incrementAll as load, add, store"""
    for p in row:
        cur = mem[p]
        yield
        if cur != 255:
            mem[p] = cur + 1
        yield


def mutant_all_no_saturation_test(mem, row):
    """word_increment_all without the test for 255: the byte wraps and carries into its neighbour"""
    for p in row:
        w, sh = p >> 2, (p & 3) * 8
        old = _wload(mem, w)
        yield
        while True:
            prev = _wcas(mem, w, old, (old + (1 << sh)) & 0xffffffff)
            yield
            if prev == old:
                break
            old = prev


def mutant_bit_load_then_or(mem, row):
    """insertAndCheck that loads the bit, decides, then ORs: two windows can both be the first writer"""
    found = 1
    for p in row:
        found &= mem[p]
        yield
        mem[p] = 1
        yield
    return found


def mutant_bit_test_after_set(mem, row):
    """insertAndCheck that sets the bit and then tests it"""
    found = 1
    for p in row:
        mem[p] = 1
        yield
        found &= mem[p]
        yield
    return found


def mutant_min_gives_up(mem, row):
    """word_increment_min that takes ANY failed word compare-and-swap for "somebody else raised my counter" and is
    done -- also when only a neighbouring counter of the word had changed"""
    mn = yield from _word_min_count(mem, row)
    if mn == 255:
        return
    for p in row:
        w, sh = p >> 2, (p & 3) * 8
        old = _wload(mem, w)
        yield
        if (old >> sh) & 0xff == mn:
            _wcas(mem, w, old, old + (1 << sh))
            yield


def mutant_min_stale_store(mem, row):
    """word_increment_min that writes `word as read + 1` back with a plain store"""
    mn = yield from _word_min_count(mem, row)
    if mn == 255:
        return
    for p in row:
        w, sh = p >> 2, (p & 3) * 8
        old = _wload(mem, w)
        yield
        if (old >> sh) & 0xff == mn:
            _wstore(mem, w, old + (1 << sh))
            yield


# ---------------------------------------------------------------------------------------------------------------
# input builders (CPU only, deterministic)
# ---------------------------------------------------------------------------------------------------------------
_UNCLEAN = b"Nn-RY\x00\xff"


def _dirty(rng, s, p_bad, at_least_one=False):
    s = np.frombuffer(s, np.uint8).copy()
    bad = rng.rand(s.size) < p_bad
    if at_least_one and p_bad and not bad.any():
        bad[rng.randint(s.size)] = True
    s[bad] = rng.choice(list(_UNCLEAN), int(bad.sum()))
    return s.tobytes()


def _acgt(rng, n):
    return bytes(rng.choice(list(b"ACGTacgt"), n).astype(np.uint8))


def contended_inputs(seed, k, unit=150, repeats=(300, 600), run=20, p_bad=0.02):
    """Buffers whose windows fight over positions, one per layout a sequence call takes
    -> [(name, buffer, starts or None, read_len)]:
      tandem     one sequence: a homopolymer and period-2 / period-3 tandem repeats (the same k-mer in adjacent
                 windows of one lane) between random stretches;
      repeatN    one read of `unit` bases N times, uniform layout (the same k-mer in many workgroups; N >= 256
                 crosses 255 inside one call);
      ragged     sequences of length 0, k-1, k, k+1, 63, 64, 65, repeats and copies of one read, by `starts`.
    `p_bad` of the bytes are unclean (the copies of a read share them)."""
    rng = np.random.RandomState(seed)
    n = k + run
    homo, per2, per3 = b"A" * n, (b"AC" * n)[:n], (b"ACG" * n)[:n]
    out = [("tandem", _dirty(rng, _acgt(rng, 40) + homo + _acgt(rng, k) + per2 + per3 + _acgt(rng, 70) + homo[: k + 3], p_bad),
            None, 0)]
    read = _dirty(rng, _acgt(rng, unit), p_bad, at_least_one=unit >= 3 * k)  # (a short read would lose all its windows)
    for r in repeats:
        out.append(("repeat%d" % r, read * r, None, unit))
    seqs = []
    for L in (0, k - 1, k, k + 1, 63, 64, 65):
        seqs += [_acgt(rng, L), read[:L] if L <= len(read) else _acgt(rng, L), homo[:L]]
    seqs += [homo, b"", per2, read, per3, read, homo, read, _acgt(rng, 3 * k), read, per2]
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    starts = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    out.append(("ragged", _dirty(rng, b"".join(seqs), p_bad), starts, 0))
    return out


def sequences(n_bytes, starts=None, read_len=0):
    """[(begin, end)] of the sequences of a buffer under a layout"""
    if starts is not None:
        s = [int(x) for x in starts]
        return list(zip(s[:-1], s[1:]))
    if read_len:
        return [(b, min(b + read_len, n_bytes)) for b in range(0, n_bytes, read_len)]
    return [(0, n_bytes)]


def clean_windows(oracle, buf, k, h, starts=None, read_len=0, seeds=None, h2=1):
    """the oracle's iterator over every sequence of the buffer -> (byte offsets of the clean windows, ascending;
    their hash rows (n, h)); with `seeds` the spaced-seed iterator, h = len(seeds) * h2"""
    cache, ps, hs = {}, [], []
    for b, e in sequences(len(buf), starts, read_len):
        s = buf[b:e]
        if s not in cache:
            r = oracle.sthash_seq(s, seeds, h2, k) if seeds else oracle.nthash_seq(s, h, k)
            cache[s] = (r[0].astype(np.int64), r[1])
        p, hv = cache[s]
        ps.append(p + b)
        hs.append(hv)
    m = len(seeds) * h2 if seeds else h
    if not ps:
        return np.zeros(0, np.int64), np.zeros((0, m), np.uint64)
    return np.concatenate(ps), np.concatenate(hs).reshape(-1, m)


def disjoint_read(oracle, size, k, h, length=150, tries=400):
    """the first RandomState(seed) read of ACGT whose windows' position sets are pairwise disjoint with h distinct
    members each -> (seed, read, hash rows); the result of any update is then order-free"""
    for seed in range(tries):
        rng = np.random.RandomState(seed)
        read = bytes(rng.choice(list(b"ACGT"), length).astype(np.uint8))
        _, hv = oracle.nthash_seq(read, h, k)
        if np.unique(positions(hv, size)).size == hv.size:
            return seed, read, hv
    raise AssertionError("no disjoint read of %d bases below seed %d (size %d, k %d, h %d)" % (length, tries, size, k, h))


def shared_words(pos, per_word):
    """words of `per_word` positions that windows of `pos` share with another window"""
    n, h = pos.shape
    key = np.unique(np.arange(n, dtype=np.int64).repeat(h) * (1 << 40) + pos.ravel() // per_word)
    return int((np.bincount(key % (1 << 40)) > 1).sum())


def crowded_words(pos, per_word):
    """words of `per_word` positions that take more than one probe, of one window or of several"""
    return int((np.bincount(np.asarray(pos).ravel() // per_word) > 1).sum())


def disjoint_rows(seed, size, h):
    """a permutation of the positions cut into rows of h, each lifted to a hash value `position + size * j` with random
    j up to the last one that fits 64 bits (the reduction modulo a size that is no power of two sees values above
    2^63) -> (n, h) uint64.  The rows share no position but nearly every word."""
    rng = np.random.RandomState(seed)
    p = rng.permutation(size)[: size // h * h]
    u = rng.randint(0, 1 << 20, p.size)
    u[:: 5] = 1 << 20  # the largest multiple that fits
    hv = [int(x) + size * ((((1 << 64) - 1 - int(x)) // size) * int(f) >> 20) for x, f in zip(p, u)]
    assert max(hv) < 2 ** 64 and max(hv) >= 2 ** 63
    return np.array(hv, dtype=np.uint64).reshape(-1, h)


def duplicated_rows(seed, rows, min_copies=1, max_copies=64):
    """every row min_copies .. max_copies times, shuffled"""
    rng = np.random.RandomState(seed)
    idx = np.arange(len(rows)).repeat(rng.randint(min_copies, max_copies + 1, len(rows)))
    return np.ascontiguousarray(rows[rng.permutation(idx)])


COUNTER_VALUES = (0, 1, 2, 127, 128, 253, 254, 255)


def prefilled_counters(seed, size):
    """saturated counters next to live ones in one word"""
    return np.random.RandomState(seed).choice(COUNTER_VALUES, size).astype(np.uint8)


def prefilled_bits(seed, size_bits):
    """random bytes: density 1/2"""
    return np.random.RandomState(seed).randint(0, 256, (size_bits + 7) // 8).astype(np.uint8)
