"""The evidence that tests/test_gpu_update_order.py can fail, and only for a reason: every checker of
tests/update_order_model.py accepts the reference's semantics under every interleaving tried (200 seeds of a random
scheduler on inputs that fight over positions), and each plausible mistake -- the mutants -- is rejected by a named
checker.  No GPU."""
import numpy as np
import pytest

import update_order_model as m

K, UNIT, SEEDS, MUTANT_SEEDS = 5, 5, 200, 96
IN_FLIGHT = (2, 4, 16, 64)  # windows started and unfinished at a time: two lanes .. one wave


@pytest.fixture(scope="module")
def rows(oracle):
    """(input index, h, size) -> positions of the clean windows of one contended input; the inputs are the GPU
    test's builder at k = 5 with a 5-base read (one window) repeated 300 and 600 times, so that a counter crosses 255
    inside one call and a scheduler step stays cheap"""
    inputs = m.contended_inputs(7, K, unit=UNIT, repeats=(300, 600), run=12)
    cache = {}

    def get(i, h, size):
        key = (i % len(inputs), h, size)
        if key not in cache:
            _, buf, starts, read_len = inputs[key[0]]
            _, hv = m.clean_windows(oracle, buf, K, h, starts, read_len)
            assert len(hv) > 100
            cache[key] = m.positions(hv, size)
        return cache[key]

    return get


def case(seed):
    """the input, the hash count, the concurrency and the filter size of a seed: every combination comes up"""
    return seed, (1, 3, 4, 5)[(seed // 4) % 4], IN_FLIGHT[(seed // 16) % 4], (64, 1000)[(seed // 64) % 2]


def m_size(size):
    return (size + 7) // 8 * 8  # CountingBloomFilter rounds its size up to a multiple of 8


def run(oracle, op, kind, pos, size, seed, in_flight):
    """simulate `op` over the windows `pos` under the schedule of `seed` and hand the result to the checker of `kind`:
    "bits" (P1-P5), "all" (A1), "min" (M1-M4) or "iac" (counting insertAndCheck); odd seeds start from a prefilled body"""
    h = pos.shape[1]
    if kind == "bits":
        before = m.prefilled_bits(seed, size) if seed % 2 else np.zeros(size // 8, np.uint8)
        mem = [int(x) for x in m.unpack_bits(before, size)]
        out = m.simulate(op, mem, pos, seed, in_flight)
        expect = before.copy()
        oracle.bf_insert(expect, size, h, pos.astype(np.uint64))
        return m.check_bit_insert_and_check(size, before, np.packbits(np.array(mem, np.uint8), bitorder="little"), expect,
                                            pos, out)
    size = m_size(size)
    before = m.prefilled_counters(seed, size) if seed % 2 else np.zeros(size, np.uint8)
    mem = [int(x) for x in before]
    thr = (1, 2, 255)[seed % 3]
    out = m.simulate(op, mem, pos, seed, in_flight, **({"thr": thr} if kind == "iac" else {}))
    after = np.array(mem, np.int64).astype(np.uint8)  # (a mutant may leave 256 in a "byte": it wraps like one)
    upper = before.copy()
    oracle.cbf_increment_all(upper, h, pos.astype(np.uint64))
    if kind == "all":
        m.check_increment_all(after, upper)
    elif kind == "min":
        m.check_increment_min(before, after, upper, pos)
    else:
        m.check_counting_insert_and_check(before, after, upper, pos, out, thr)


# the word-CAS forms are this file's own controls for the word-level mutants: a quarter of the seeds
FAITHFUL = [("bit insertAndCheck", m.ref_bit_insert_and_check, "bits", SEEDS),
            ("incrementAll", m.ref_increment_all, "all", SEEDS),
            ("incrementAll, word CAS", m.word_increment_all, "all", SEEDS // 4),
            ("incrementMin", m.ref_increment_min, "min", SEEDS),
            ("incrementMin, word CAS", m.word_increment_min, "min", SEEDS // 4),
            ("counting insertAndCheck", m.ref_counting_insert_and_check, "iac", SEEDS)]


@pytest.mark.parametrize("name,op,kind,seeds", FAITHFUL, ids=[f[0] for f in FAITHFUL])
def test_checkers_accept_every_interleaving_of_the_reference(oracle, rows, name, op, kind, seeds):
    for seed in range(seeds):
        i, h, in_flight, size = case(seed)
        try:
            run(oracle, op, kind, rows(i, h, size if kind == "bits" else m_size(size)), size, seed, in_flight)
        except m.ContractViolation as e:
            pytest.fail("%s, seed %d (input %d, h %d, %d in flight, size %d): %s" % (name, seed, i % 4, h, in_flight, size, e))


# (mutant, its operation, the checker it faces, the property that must be among those that reject it)
MUTANTS = [("incrementAll: load, add, store", m.mutant_all_lost_update, "all", "A1"),
           ("incrementAll: word CAS without the 255 test", m.mutant_all_no_saturation_test, "all", "A1"),
           ("insertAndCheck: load, decide, OR", m.mutant_bit_load_then_or, "bits", "P5"),
           ("insertAndCheck: test after set", m.mutant_bit_test_after_set, "bits", "P3"),
           ("incrementMin: done after a CAS that a neighbour failed", m.mutant_min_gives_up, "min", "M3"),
           ("incrementMin: stale word stored without CAS", m.mutant_min_stale_store, "min", "M3")]


@pytest.mark.parametrize("name,op,kind,prop", MUTANTS, ids=[x[0] for x in MUTANTS])
def test_each_mutant_is_rejected_by_a_named_checker(oracle, rows, name, op, kind, prop):
    rejected = {}
    for seed in range(MUTANT_SEEDS):
        i, h, in_flight, size = case(seed)
        try:
            run(oracle, op, kind, rows(i, h, size if kind == "bits" else m_size(size)), size, seed, in_flight)
        except m.ContractViolation as e:
            rejected.setdefault(e.prop, []).append(seed)
    by = ", ".join("%s (%d of %d seeds)" % (p, len(s), MUTANT_SEEDS) for p, s in sorted(rejected.items()))
    print("%-58s rejected by %s" % (name, by or "nothing"))
    assert prop in rejected, (name, rejected)


def test_a_carry_into_a_neighbour_nobody_probes_is_named_by_m1(oracle):
    # the word-level mistake M1's third clause exists for, on the smallest example: counters [255, 7] in one word, one
    # window on counter 0 -- an unguarded +1 on the word wraps counter 0 and carries into counter 1
    before = np.array([255, 7, 0, 0, 0, 0, 0, 0], np.uint8)
    after = np.array([0, 8, 0, 0, 0, 0, 0, 0], np.uint8)
    pos = np.array([[0]])
    with pytest.raises(m.ContractViolation) as e:
        m.check_increment_min(before, after, before, pos)
    assert e.value.prop == "M1"
    with pytest.raises(m.ContractViolation) as e:
        m.check_increment_min(before, np.array([255, 8, 0, 0, 0, 0, 0, 0], np.uint8), before, pos)
    assert e.value.prop == "M1" and "probed by no window" in str(e.value)


def finished(g):
    try:
        next(g)
    except StopIteration:
        return True
    return False


def test_one_call_may_raise_a_repeated_kmer_by_one_only_when_each_copy_wins_another_counter(oracle):
    # two windows of one k-mer with h = 2: both read minimum 0; a wins the compare-and-swap on counter 1, b loses it
    # there but wins on counter 6, a loses on counter 6.  Each has made an update, so both are DONE, and the k-mer's
    # minimum is 1 after two occurrences.  M3 asks for + 1, not for + multiplicity -- in the reference too.
    mem = [0] * 8
    a, b = m.ref_increment_min(mem, [1, 6]), m.ref_increment_min(mem, [1, 6])
    for g in (a, b, a, b):  # the two minCount loads of each
        assert not finished(g)
    for g in (a, b, b, a):  # the compare-and-swaps: a on 1 (wins), b on 1 (loses), b on 6 (wins), a on 6 (loses)
        assert not finished(g)
    assert finished(a) and finished(b)  # nothing left to run: this is the final state
    assert mem == [0, 1, 0, 0, 0, 0, 1, 0]
    m.check_increment_min(np.zeros(8, np.uint8), np.array(mem, np.uint8), np.array([0, 2, 0, 0, 0, 0, 2, 0], np.uint8),
                          np.array([[1, 6], [1, 6]]))
    # a window that won nothing is not done: with the swaps in the order a, b, a, b the second copy loses both, reads the
    # minimum again and raises it to 2
    mem = [0] * 8
    a, b = m.ref_increment_min(mem, [1, 6]), m.ref_increment_min(mem, [1, 6])
    for g in (a, b, a, b, a, b, a, b):
        assert not finished(g)
    assert finished(a) and not finished(b)
    while not finished(b):
        pass
    assert mem == [0, 2, 0, 0, 0, 0, 2, 0]


@pytest.mark.parametrize("op", [m.ref_increment_min, m.word_increment_min], ids=["reference", "word CAS"])
def test_with_one_hash_the_minimum_rises_by_the_full_multiplicity(op):
    # h = 1: a window's only compare-and-swap either makes its update or is repeated on a fresh read, so no occurrence
    # is lost under any schedule: n copies -> + n, up to 255
    for seed in range(40):
        n = (1, 2, 7, 100, 254, 255, 256, 300)[seed % 8]
        mem = [0, 0, 3, 254, 0, 0, 0, 0]
        m.simulate(op, mem, [[2]] * n + [[5]], seed, in_flight=(2, 8, 64)[seed % 3])
        assert mem == [0, 0, min(3 + n, 255), 254, 0, 1, 0, 0], (seed, n)
