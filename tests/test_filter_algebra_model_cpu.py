"""tests/filter_algebra_model.py pinned on the host, against filters the oracle builds: the fold of a bit filter built at m
is the filter built at m / d; the same for 8-bit counters under cbf_increment_all; union and add-merge equal building from
the concatenated reads; threshold_bits answers as the counting query does.  The exact and the vectorised combine agree.
The GPU tests (test_gpu_filter_algebra.py) then hold the kernels to this model."""
import numpy as np
import pytest

import filter_algebra_model as fm

H, K, L = 3, 25, 100


def built_bits(o, bits, reads):
    f = np.zeros(bits // 8, np.uint8)
    for r in reads.reshape(-1, L):
        o.bf_insert_seq(f, bits, H, K, r.tobytes())
    return f


def built_counters(o, nbytes, reads):
    c = np.zeros(nbytes, np.uint8)
    for r in reads.reshape(-1, L):
        _, hv = o.nthash_seq(r.tobytes(), H, K)
        o.cbf_increment_all(c, H, hv)
    return c


@pytest.mark.parametrize("d", [2, 3, 5, 64])
def test_fold_of_a_built_bit_filter_is_the_filter_built_smaller(oracle, d):
    reads = oracle.synth_reads(3, 0, 60, L)
    small_bits = 8 * 1031  # an odd number of bytes: slices at every alignment
    big = built_bits(oracle, small_bits * d, reads)
    small = built_bits(oracle, small_bits, reads)
    assert small.any() and (fm.fold(big, d, 0) == small).all()


@pytest.mark.parametrize("d", [2, 3, 16])
def test_fold_of_increment_all_counters(oracle, d):
    one = oracle.synth_reads(4, 0, 1, L)
    reads = np.concatenate([oracle.synth_reads(5, 0, 30, L)] + [one] * 300)  # byte counters saturate
    nbytes = 1032
    big = built_counters(oracle, nbytes * d, reads)
    small = built_counters(oracle, nbytes, reads)
    assert small.max() == 255 and (fm.fold(big, d, 1) == small).all()


def test_union_and_add_merge_equal_building_from_all_reads(oracle):
    one = oracle.synth_reads(6, 0, 1, L)
    r1 = np.concatenate([oracle.synth_reads(7, 0, 40, L)] + [one] * 150)
    r2 = np.concatenate([oracle.synth_reads(8, 0, 30, L)] + [one] * 150)
    both = np.concatenate([r1, r2])
    bits = 1 << 15
    a, b = built_bits(oracle, bits, r1), built_bits(oracle, bits, r2)
    body, pop = fm.combine(a, [b], fm.OR, 0)
    want = built_bits(oracle, bits, both)
    assert (body == want).all() and pop == oracle.bf_popcount(want, bits)
    ca, cb = built_counters(oracle, 1 << 15, r1), built_counters(oracle, 1 << 15, r2)
    body, pop = fm.combine(ca, [cb], fm.ADD, 1)
    want = built_counters(oracle, 1 << 15, both)
    assert want.max() == 255 and ca.max() < 255 and cb.max() < 255  # only the sum saturates
    assert (body == want).all() and pop == oracle.cbf_popcount(want)


def test_threshold_bits_answers_like_the_counting_query(oracle):
    once, twice = oracle.synth_reads(9, 0, 20, L), oracle.synth_reads(10, 0, 20, L)
    c = built_counters(oracle, 2048, np.concatenate([once, twice, twice]))
    for t in (1, 2, 3):
        bits = fm.threshold_bits(c, t, 1)
        assert int(np.unpackbits(bits).sum()) == oracle.cbf_filtered_popcount(c, t)
        for r in np.concatenate([once, twice, oracle.synth_reads(11, 0, 10, L)]).reshape(-1, L):
            _, hv = oracle.nthash_seq(r.tobytes(), H, K)
            _, contains = oracle.cbf_query(c, H, t, hv)
            assert (oracle.bf_contains(bits, 2048, H, hv) == contains).all()


@pytest.mark.parametrize("cb", [1, 2, 4, 8])
def test_exact_and_vectorised_combine_agree(cb):
    rng = np.random.default_rng(cb)
    mx = fm.counter_max(cb)
    edge = np.array([0, 1, mx - 1, mx, mx // 2, mx // 2 + 1, 0xFFFFFFFF & mx], dtype="<u%d" % cb)
    bodies = [edge[rng.integers(0, len(edge), 512)].view(np.uint8) for _ in range(4)]
    for op in fm.COUNTER_OPS:
        for n in (1, 3):
            a, pa = fm.combine(bodies[0], bodies[1 : 1 + n], op, cb)
            b, pb = fm.combine_fast(bodies[0], bodies[1 : 1 + n], op, cb)
            assert (a == b).all() and pa == pb
    # and by hand: saturation never wraps, for every width
    x = np.array([mx, mx - 1, 1, 0], dtype="<u%d" % cb).view(np.uint8)
    y = np.array([mx, 2, mx - 1, 0], dtype="<u%d" % cb).view(np.uint8)
    body, pop = fm.combine(x, [y], fm.ADD, cb)
    assert body.view("<u%d" % cb).tolist() == [mx, mx, mx, 0] and pop == 3
    assert fm.fold(np.concatenate([x, y]), 2, cb).view("<u%d" % cb).tolist() == [mx, mx, mx, 0]
