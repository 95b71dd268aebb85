"""calcFrameProbs (MIBloomFilter.hpp:664-679, over calcProbSingleFrame :65-77 and nChoosek :781-796) restated in Python
floats: IEEE doubles, the same order of operations, math.pow (the C library's pow).  Pinned to the reference bit for bit
by tests/test_mibf_frame_probs_vs_ref.py; the checker of btlbf_mibf_frame_probs in tests/test_gpu_mibf_frame_probs.py."""
import math


def n_choose_k(n, k):
    """the reference's nChoosek: the running product is an int, multiplied and divided as unsigned"""
    if k > n:
        return 0
    if k * 2 > n:
        k = n - k
    if k == 0:
        return 1
    result = n
    for i in range(2, k + 1):
        result = (result * (n - i + 1)) & 0xFFFFFFFF
        result //= i
    return result


def prob_single_frame(occupancy, h, freq, allowed_miss):
    total = 0.0
    for i in range(h - allowed_miss, h + 1):
        prob = float(n_choose_k(h, i))
        prob *= math.pow(occupancy, float(i))
        prob *= math.pow(1.0 - occupancy, float(h - i))
        prob *= 1.0 - math.pow(1.0 - freq, float(i))
        total += prob
    return total


def frame_probs_model(counts, pop, size, h, allowed_miss):
    """counts: getIDCounts over len(counts) bins; pop / size: set bits and length of the bit vector.
    -> frameProbs as a list; entry 0 is None (the reference leaves frameProbs[0] as it was)"""
    assert 0 <= allowed_miss <= h
    occupancy = float(pop) / float(size)
    total = sum(int(c) for c in counts[1:])
    assert total > 0
    return [None] + [prob_single_frame(occupancy, h, float(int(c)) / float(total), allowed_miss) for c in counts[1:]]


def sat_prop_model(counts, saturated):
    return float(saturated) / float(sum(int(c) for c in counts[1:]))
