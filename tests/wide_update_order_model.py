"""csrc/wide_counter.hpp restated for the interleaving simulator of tests/update_order_model.py (simulate): generators
that perform exactly ONE atomic memory operation per step, for counters of 16, 32 and 64 bits.  No GPU import.

`mem` is a list of Python ints, one per counter.  A 16-bit counter is halfword p & 1 of 32-bit word p >> 1 and only the
word can be compared and swapped (WideCtr<2>); a 32- or 64-bit counter is compared and swapped itself.  On top of the
three per-counter operations -- read_fresh, inc_sat, cas_inc -- stand wide_increment_min, incrementAll and the counting
insertAndCheck of the hash-row kernel (minimum, report, incrementMin), and next to them the reference's own per-counter
forms (CountingBloomFilter.hpp:135-183) with MAX = 2^bits - 1.  Every mutant is one of these with one plausible mistake.

tests/test_wide_update_order_cpu.py runs all of them against the checkers of tests/wide_counter_model.py: the evidence
that tests/test_gpu_wide_update_order.py can fail, and only for a reason."""
import numpy as np

import update_order_model as uo
import wide_counter_model as wm


# ---------------------------------------------------------------------------------------------------------------
# the reference, step by step (update_order_model.ref_* with MAX for 255)
# ---------------------------------------------------------------------------------------------------------------
def ref_increment_all(mem, row, bits):
    mx = wm.max_of(bits)
    for p in row:
        while True:
            cur = mem[p]  # currentVal = m_filter[pos]
            yield
            if cur == mx:  # newVal < currentVal
                break
            ok = mem[p] == cur  # __sync_bool_compare_and_swap
            if ok:
                mem[p] = cur + 1
            yield
            if ok:
                break


def _ref_min_count(mem, row, mx):
    mn = mx
    for p in row:
        mn = min(mn, mem[p])
        yield
    return mn


def ref_increment_min(mem, row, bits):
    mx = wm.max_of(bits)
    mn = yield from _ref_min_count(mem, row, mx)
    done = False
    while not done:
        if mn == mx:  # minVal > newVal
            return
        for p in row:
            if mem[p] == mn:  # __sync_bool_compare_and_swap(minVal, newVal)
                mem[p] = mn + 1
                done = True
            yield
        if not done:
            mn = yield from _ref_min_count(mem, row, mx)


def ref_counting_insert_and_check(mem, row, bits, thr=1):
    found = int((yield from _ref_min_count(mem, row, wm.max_of(bits))) >= thr)
    yield from ref_increment_min(mem, row, bits)
    return found


# ---------------------------------------------------------------------------------------------------------------
# WideCtr<BYTES>: the three operations on one counter.  `sh_of` is the halfword's shift (a mutant passes a wrong one)
# ---------------------------------------------------------------------------------------------------------------
def _sh(p):
    return (p & 1) * 16


def _wload(mem, w):
    return mem[2 * w] | mem[2 * w + 1] << 16


def _wstore(mem, w, v):
    mem[2 * w], mem[2 * w + 1] = v & 0xffff, (v >> 16) & 0xffff


def _wcas(mem, w, old, new):
    cur = _wload(mem, w)
    if cur == old:
        _wstore(mem, w, new)
    return cur


def read_fresh(mem, p, bits, sh_of=_sh):
    if bits == 16:
        v = (_wload(mem, p >> 1) >> sh_of(p)) & 0xffff  # agent_load of the word
    else:
        v = mem[p]
    yield
    return v


def inc_sat(mem, p, bits, sh_of=_sh, is_max=None):
    """saturating +1; `is_max(v)` is the MAX test (a mutant passes a wrong one)"""
    mx = wm.max_of(bits)
    is_max = is_max or (lambda v: v == mx)
    if bits == 16:
        w, sh = p >> 1, sh_of(p)
        old = _wload(mem, w)
        yield
        while True:
            if is_max((old >> sh) & 0xffff):
                return
            prev = _wcas(mem, w, old, (old + (1 << sh)) & 0xffffffff)
            yield
            if prev == old:
                return
            old = prev
    old = mem[p]
    yield
    while not is_max(old):
        prev = mem[p]  # atomicCAS(c, old, old + 1)
        if prev == old:
            mem[p] = (old + 1) & mx
        yield
        if prev == old:
            return
        old = prev


def cas_inc(mem, p, expect, bits, sh_of=_sh):
    """expect -> expect + 1; -> whether this call made the change"""
    if bits == 16:
        w, sh = p >> 1, sh_of(p)
        old = _wload(mem, w)
        yield
        while True:
            if (old >> sh) & 0xffff != expect:
                return False
            prev = _wcas(mem, w, old, old + (1 << sh))
            yield
            if prev == old:
                return True
            old = prev
    ok = mem[p] == expect  # one atomicCAS on the counter
    if ok:
        mem[p] = expect + 1
    yield
    return ok


# ---------------------------------------------------------------------------------------------------------------
# the kernels' forms
# ---------------------------------------------------------------------------------------------------------------
def wide_increment_min(mem, row, bits, sh_of=_sh, less=None, is_max=None):
    """wide_increment_min<BYTES>; `less(v, mn)` and `is_max(mn)` are the comparisons (mutants pass wrong ones)"""
    mx = wm.max_of(bits)
    less = less or (lambda v, mn: v < mn)
    is_max = is_max or (lambda v: v == mx)
    while True:
        mn = mx
        for p in row:
            v = yield from read_fresh(mem, p, bits, sh_of)
            mn = v if less(v, mn) else mn
        if is_max(mn):
            return
        done = False
        for p in row:
            done |= yield from cas_inc(mem, p, mn, bits, sh_of)
        if done:
            return


def wide_increment_all(mem, row, bits):
    for p in row:
        yield from inc_sat(mem, p, bits)


def wide_insert_and_check(mem, row, bits, thr=1):
    """wide_row_op, H_CBF_INSERT_CHECK: the minimum over fresh reads, the report, then incrementMin"""
    mn = wm.max_of(bits)
    for p in row:
        mn = min(mn, (yield from read_fresh(mem, p, bits)))
    found = int(mn >= thr)
    yield from wide_increment_min(mem, row, bits)
    return found


# ---------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------
def mutant_all_no_max_test(mem, row, bits):
    """incrementAll without the MAX test: 16 bits, the halfword at 0xffff wraps and the low one carries into its
    neighbour; 32 / 64 bits, the counter wraps to 0"""
    for p in row:
        yield from inc_sat(mem, p, bits, is_max=lambda v: False)


def mutant_all_lost_update(mem, row, bits):
    """incrementAll as load, add, store (16 bits: of the word, as the hardware would have to do it)"""
    mx = wm.max_of(bits)
    for p in row:
        if bits == 16:
            w, sh = p >> 1, _sh(p)
            old = _wload(mem, w)
            yield
            if (old >> sh) & 0xffff != mx:
                _wstore(mem, w, old + (1 << sh))
            yield
        else:
            cur = mem[p]
            yield
            if cur != mx:
                mem[p] = cur + 1
            yield


def mutant_all_max_test_through_a_byte(mem, row, bits):
    """incrementAll whose MAX test looks at the low byte: a counter at 0xff, 0x1ff, ... is taken for saturated"""
    for p in row:
        yield from inc_sat(mem, p, bits, is_max=lambda v: v & 0xff == 0xff)


def mutant_min_gives_up(mem, row, bits):
    """16 bits: incrementMin that takes ANY failed word swap for "somebody else raised my counter" and is done -- also
    when only the neighbouring halfword had changed"""
    assert bits == 16
    mn = 0xffff
    for p in row:
        mn = min(mn, (yield from read_fresh(mem, p, bits)))
    if mn == 0xffff:
        return
    for p in row:
        w, sh = p >> 1, _sh(p)
        old = _wload(mem, w)
        yield
        if (old >> sh) & 0xffff == mn:
            _wcas(mem, w, old, old + (1 << sh))
            yield


def mutant_min_stale_store(mem, row, bits):
    """16 bits: incrementMin that writes `word as read + 1` back with a plain store"""
    assert bits == 16
    mn = 0xffff
    for p in row:
        mn = min(mn, (yield from read_fresh(mem, p, bits)))
    if mn == 0xffff:
        return
    for p in row:
        w, sh = p >> 1, _sh(p)
        old = _wload(mem, w)
        yield
        if (old >> sh) & 0xffff == mn:
            _wstore(mem, w, old + (1 << sh))
            yield


def mutant_min_through_a_byte(mem, row, bits):
    """incrementMin whose `v < mn` compares the low bytes: 0x100 counts as less than 0xff"""
    yield from wide_increment_min(mem, row, bits, less=lambda v, mn: v & 0xff < mn & 0xff)


def mutant_min_max_test_through_a_byte(mem, row, bits):
    """incrementMin whose MAX test looks at the low byte of the minimum: a minimum of 0xff is taken for saturated"""
    yield from wide_increment_min(mem, row, bits, is_max=lambda v: v & 0xff == 0xff)


def mutant_min_through_32_bits(mem, row, bits):
    """64 bits: `v < mn` on the low 32 bits: 2^32 counts as less than 2^32 - 1"""
    assert bits == 64
    yield from wide_increment_min(mem, row, bits, less=lambda v, mn: v & 0xffffffff < mn & 0xffffffff)


def mutant_min_max_test_through_32_bits(mem, row, bits):
    """64 bits: the MAX test on the low 32 bits of the minimum: 2^32 - 1 is taken for saturated"""
    assert bits == 64
    yield from wide_increment_min(mem, row, bits, is_max=lambda v: v & 0xffffffff == 0xffffffff)


def mutant_min_one_pass(mem, row, bits):
    """incrementMin without the outer loop: a window all of whose swaps failed -- others had raised its counters -- is
    done without an update of its own"""
    mx = wm.max_of(bits)
    mn = mx
    for p in row:
        mn = min(mn, (yield from read_fresh(mem, p, bits)))
    if mn == mx:
        return
    for p in row:
        yield from cas_inc(mem, p, mn, bits)


def _wrong_sh(p):
    return ((p >> 1) & 1) * 16


def mutant_min_wrong_shift_bit(mem, row, bits):
    """16 bits: the halfword's shift taken from bit 1 of the index instead of bit 0"""
    assert bits == 16
    yield from wide_increment_min(mem, row, bits, sh_of=_wrong_sh)


def mutant_all_wrong_shift_bit(mem, row, bits):
    assert bits == 16
    for p in row:
        yield from inc_sat(mem, p, bits, sh_of=_wrong_sh)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
SIZES = (4, 32, 500)  # counters
N_WINDOWS, N_DISTINCT, H = 200, 25, 3
IN_FLIGHT = (2, 64)
# the values around which a comparison or a MAX test on the low 32 bits of a 64-bit counter goes wrong; none of
# wm.prefill_values(64) lies there (they are below 2^9 or above 2^64 - 4, where the low half orders as the whole does)
AROUND_2_32 = (0xfffffffe, 0xffffffff, 0x100000000)


def windows(seed, size):
    """N_WINDOWS rows of H positions drawn from N_DISTINCT distinct hash rows -> (200, 3) int64"""
    rng = np.random.RandomState(7000 + seed)
    hv = rng.randint(0, 1 << 62, (N_DISTINCT, H)).astype(np.uint64)
    return wm.positions(hv[rng.randint(0, N_DISTINCT, N_WINDOWS)], size)


LOW = "low"  # as `extra`: only the prefill values that no call here can raise to MAX, so that M4 is in force


def body(seed, size, bits, extra=()):
    """`size` counters drawn from wm.prefill_values(bits) (+ extra; LOW: from {0, 1, 0xff, 0x100} alone) -> [int]"""
    vals = wm.prefill_values(bits)[:4] if extra == LOW else wm.prefill_values(bits) + tuple(extra)
    rng = np.random.RandomState(9000 + seed)
    return [vals[i] for i in rng.randint(0, len(vals), size)]


# ---------------------------------------------------------------------------------------------------------------
# inputs of the GPU tests (tests/test_gpu_wide_update_order.py)
# ---------------------------------------------------------------------------------------------------------------
TILE = 2048  # windows per tile of wide_seq_kernel: 256 lanes of 8


def enlarged_ragged(seed, buf, starts, times=6):
    """the sequences of a ragged buffer `times` times over, shuffled, with their own starts -> (buffer, starts): several
    tiles, so that the kernel's search of `starts` begins inside the list on all tiles but the first"""
    seqs = [bytes(buf[b:e]) for b, e in uo.sequences(len(buf), starts)] * times
    order = np.random.RandomState(seed).permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    return b"".join(seqs), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


def straddling(clean, k):
    """clean windows that start in the last k - 1 offsets of a tile: their bases lie in two tiles"""
    return int((np.asarray(clean, np.int64) % TILE > TILE - k).sum())
