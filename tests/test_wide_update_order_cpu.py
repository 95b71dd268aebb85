"""The evidence that tests/test_gpu_wide_update_order.py can fail, and only for a reason: the wide checkers of
tests/wide_counter_model.py (check_increment_all, check_increment_min, check_counting_insert_and_check: A1, M1-M4, C0-C1
with MAX = 2^bits - 1) accept every seeded schedule of the correct algorithm -- the reference's per-counter form and the
kernels' form of csrc/wide_counter.hpp, where a 16-bit counter is swapped through its 32-bit word -- and reject each
plausible mistake by a named property.  tests/wide_update_order_model.py has the generators.  No GPU.

Shapes: filters of 4, 32 and 500 counters prefilled from prefill_values(bits); 200 windows of h = 3 drawn from 25
distinct rows; 2 and 64 windows in flight; 12 seeds: 72 runs per form and width (the mutants: 18 seeds, 108 runs)."""
import numpy as np
import pytest

import update_order_model as uo
import wide_counter_model as wm
import wide_update_order_model as w

WIDTHS = (16, 32, 64)
SEEDS = tuple(range(12))
RUNS = [(seed, size, fl) for seed in SEEDS for size in w.SIZES for fl in w.IN_FLIGHT]
# the mutants face six seeds more, chosen because the two that show only in a rare schedule -- a word swap or a word
# store that falls between a neighbour's load and its swap -- are caught there (M3 under seeds 3 and 48, M4 under the
# others, on the 4-counter body that holds no MAX); the list is fixed, and a mutant that survives it fails the test
MUTANT_SEEDS = SEEDS + (14, 19, 42, 47, 48, 54)
MUTANT_RUNS = [(seed, size, fl) for seed in MUTANT_SEEDS for size in w.SIZES for fl in w.IN_FLIGHT]


def run(op, kind, bits, seed, size, in_flight, extra=()):
    """simulate `op` over the windows of `seed` on a prefilled body under the schedule of `seed` and hand the result to
    the checker of `kind`: "all" (A1), "min" (M1-M4) or "iac" (C0-C1, M1-M4)"""
    mx = wm.max_of(bits)
    pos = w.windows(seed, size)
    mem = w.body(seed, size, bits, extra)
    before = np.array(mem, dtype=np.uint64)
    thr = (1, 2, 256, min(mx, 0xffffffff))[seed % 4]
    out = uo.simulate(op, mem, pos, seed, in_flight, bits=bits, **({"thr": thr} if kind == "iac" else {}))
    assert all(0 <= v <= mx for v in mem)
    after = np.array(mem, dtype=np.uint64)
    upper = wm.increment_all_exact(before, pos, mx)
    if kind == "all":
        wm.check_increment_all(after, upper)
    elif kind == "min":
        wm.check_increment_min(before, after, upper, pos, mx)
    else:
        wm.check_counting_insert_and_check(before, after, upper, pos, out, thr, mx)


def test_the_inputs_fight_over_counters_and_over_words():
    for seed, size, _ in RUNS:
        pos = w.windows(seed, size)
        assert pos.shape == (w.N_WINDOWS, w.H) and len(np.unique(pos, axis=0)) <= w.N_DISTINCT
        assert np.bincount(pos.ravel()).max() > w.H  # a counter that several windows probe
        assert uo.shared_words(pos, 2) > 0  # 16 bits: a word whose halves belong to different windows
    for bits in WIDTHS:  # every prefill value occurs, MAX and the values around a byte's end among them
        vals = set()
        for seed in SEEDS:
            vals |= set(w.body(seed, 500, bits))
        assert vals == set(wm.prefill_values(bits))
    assert wm.increment_all_exact([0, 5, 2 ** 64 - 2, 2 ** 64 - 1], [[0, 2, 2], [3, 2, 0]], 2 ** 64 - 1).tolist() == \
        [2, 5, 2 ** 64 - 1, 2 ** 64 - 1]


FAITHFUL = [("incrementAll, reference form", w.ref_increment_all, "all"),
            ("incrementAll, kernel form", w.wide_increment_all, "all"),
            ("incrementMin, reference form", w.ref_increment_min, "min"),
            ("incrementMin, kernel form", w.wide_increment_min, "min"),
            ("insertAndCheck, reference form", w.ref_counting_insert_and_check, "iac"),
            ("insertAndCheck, kernel form", w.wide_insert_and_check, "iac")]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("name,op,kind", FAITHFUL, ids=[f[0] for f in FAITHFUL])
def test_checkers_accept_every_schedule_of_the_correct_forms(name, op, kind, bits):
    for seed, size, fl in RUNS:
        # (the LOW body: no counter can reach MAX, so M4 -- n .. h * n successful swaps -- is in force on every run)
        for extra in ((), w.LOW, w.AROUND_2_32) if bits == 64 else ((), w.LOW):
            try:
                run(op, kind, bits, seed, size, fl, extra)
            except uo.ContractViolation as e:
                pytest.fail("%s, %d bits, seed %d, %d counters, %d in flight: %s" % (name, bits, seed, size, fl, e))


# (mutant, its operation, the checker it faces, the widths at which it is a mistake of its own, the property that must
# be among those that reject it, extra prefill values).  What is left out, and why:
#   * "gives up" and "plain store" at 32 / 64 bits: the counter itself is swapped, so a failed swap does mean that the
#     own counter has changed -- that is the reference's form -- and there is no neighbour to write over.  What can
#     still go wrong there is the outer loop: that mutant runs at every width, on the LOW body, where M4 counts swaps;
#   * the wrong shift bit has no meaning without halfwords;
#   * the 32-bit comparisons of a 64-bit counter need a counter between 2^32 - 2 and 2^32 to go wrong, which
#     prefill_values(64) does not hold: those two runs draw from prefill_values(64) + AROUND_2_32 (the correct forms
#     above run on that body as well).
MUTANTS = [
    ("incrementAll without the MAX test", w.mutant_all_no_max_test, "all", WIDTHS, "A1", ()),
    ("incrementAll as load, add, store", w.mutant_all_lost_update, "all", WIDTHS, "A1", ()),
    ("incrementAll, MAX test through a byte", w.mutant_all_max_test_through_a_byte, "all", WIDTHS, "A1", ()),
    ("incrementAll, shift from the wrong index bit", w.mutant_all_wrong_shift_bit, "all", (16,), "A1", ()),
    ("incrementMin gives up on any failed word swap", w.mutant_min_gives_up, "min", (16,), "M3", ()),
    ("incrementMin stores the word without a swap", w.mutant_min_stale_store, "min", (16,), "M3", ()),
    ("incrementMin without the outer loop", w.mutant_min_one_pass, "min", WIDTHS, "M4", w.LOW),
    ("incrementMin, minimum through a byte", w.mutant_min_through_a_byte, "min", WIDTHS, "M3", ()),
    ("incrementMin, MAX test through a byte", w.mutant_min_max_test_through_a_byte, "min", WIDTHS, "M3", ()),
    ("incrementMin, minimum through 32 bits", w.mutant_min_through_32_bits, "min", (64,), "M3", w.AROUND_2_32),
    ("incrementMin, MAX test through 32 bits", w.mutant_min_max_test_through_32_bits, "min", (64,), "M3", w.AROUND_2_32),
    ("incrementMin, shift from the wrong index bit", w.mutant_min_wrong_shift_bit, "min", (16,), "M1", ()),
]
MUTANT_CASES = [(m[0], m[1], m[2], bits, m[4], m[5]) for m in MUTANTS for bits in m[3]]


@pytest.mark.parametrize("name,op,kind,bits,prop,extra", MUTANT_CASES, ids=["%s-u%d" % (c[0], c[3]) for c in MUTANT_CASES])
def test_each_mutant_is_rejected_by_a_named_property(name, op, kind, bits, prop, extra):
    rejected = {}
    for seed, size, fl in MUTANT_RUNS:
        try:
            run(op, kind, bits, seed, size, fl, extra)
        except uo.ContractViolation as e:
            rejected.setdefault(e.prop, []).append((seed, size, fl))
    by = ", ".join("%s (%d of %d runs)" % (p, len(s), len(MUTANT_RUNS)) for p, s in sorted(rejected.items()))
    print("%-48s u%-2d rejected by %s" % (name, bits, by or "nothing"))
    assert rejected, "%s, %d bits: survived all %d runs" % (name, bits, len(MUTANT_RUNS))
    assert prop in rejected, (name, bits, by)


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_wrap_at_max_is_named(bits):
    # the smallest examples: one window on counter 0, which is at MAX beside a live neighbour
    mx = wm.max_of(bits)
    before = np.array([mx, 7, 0, 0], np.uint64)
    pos = np.array([[0]])
    for after in ([0, 8, 0, 0], [mx, 8, 0, 0], [0, 7, 0, 0]):  # carry and wrap; the carry alone; the wrap alone
        with pytest.raises(uo.ContractViolation) as e:
            wm.check_increment_min(before, np.array(after, np.uint64), before, pos, mx)
        assert e.value.prop == "M1"
        with pytest.raises(uo.ContractViolation) as e:
            wm.check_increment_all(np.array(after, np.uint64), before)
        assert e.value.prop == "A1"
    # the halfword model does carry: an unguarded + 1 on the word [0xffff, 7] gives [0, 8]
    mem = [0xffff, 7, 0, 0]
    uo.simulate(w.mutant_all_no_max_test, mem, [[0]], 0, 1, bits=16)
    assert mem == [0, 8, 0, 0]
    mem = [7, 0xffff, 0, 0]
    uo.simulate(w.wide_increment_all, mem, [[0], [1], [0]], 0, 2, bits=16)
    assert mem == [9, 0xffff, 0, 0]


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("op", [w.ref_increment_min, w.wide_increment_min], ids=["reference", "kernel"])
def test_with_one_hash_the_minimum_rises_by_the_full_multiplicity(op, bits):
    # h = 1: no occurrence is lost under any schedule -- n copies give + n up to MAX; the neighbour in the word (16 bits)
    # is raised by other windows all the while
    mx = wm.max_of(bits)
    for seed in range(24):
        n = (1, 2, 7, 100, 300)[seed % 5]
        mem = [0, 0, mx - 5, 254, 0, 0, 0, 0]
        uo.simulate(op, mem, [[2], [3]] * n + [[5]], seed, in_flight=(2, 8, 64)[seed % 3], bits=bits)
        assert mem == [0, 0, min(mx - 5 + n, mx), 254 + n, 0, 1, 0, 0], (seed, n)
