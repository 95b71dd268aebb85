"""btlbf_mibf_frame_probs / MIBloomFilter.calcFrameProbs on the GPU's miBF against tests/mibf_frame_probs_model.py (pinned
to the reference's calcFrameProbs bit for bit by tests/test_mibf_frame_probs_vs_ref.py) over the same object's
getIDCounts / getPop / size: exactly, since both sides are IEEE doubles through the same libm on one machine."""
import ctypes as C

import numpy as np
import pytest

from mibf_frame_probs_model import frame_probs_model, sat_prop_model
from test_gpu_mibf_classify import Case, bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(bf):  # noqa: F811
    return Case(bf, "C5", 2, 40)  # the seeded configuration of the classify tests: h = 4, ids 1..40


def test_equals_the_model_exactly(case):
    m, n = case.m, case.n_ids
    counts, saturated = m.getIDCounts(n)
    assert counts[1:].sum() > 0 and saturated > 0 and int((case.data & 0x7FFF).max()) == n - 1
    for a in (0, 1):
        probs, sat_prop = m.calcFrameProbs(n, a)
        exp = frame_probs_model(counts, m.getPop(), m.size(), m.getHashNum(), a)
        assert [float(x) for x in probs[1:]] == exp[1:], a
        assert sat_prop == sat_prop_model(counts, saturated) == float(saturated) / float(int(counts[1:].sum()))
        assert len(set(exp[1:])) >= 2 and all(0.0 < x < 1.0 for x in exp[1:])
    # more bins than ids: the extra ones have no entry and probability 0
    probs, _ = m.calcFrameProbs(n + 3, 1)
    assert [float(x) for x in probs[1:n]] == exp[1:] and not probs[n:].any()
    assert m.calcProbSingleFrame(0.25, 4, 0.125, 1) == frame_probs_model([0, 1, 7], 1, 4, 4, 1)[1]


def test_entry_zero_is_untouched(case, bf):  # noqa: F811
    L = bf._lib.load()
    probs = np.full(case.n_ids, -7.5)
    sat = C.c_double(-1.0)
    assert L.btlbf_mibf_frame_probs(case.m._h, 0, C.c_void_p(probs.ctypes.data), case.n_ids, C.byref(sat)) == 0
    assert probs[0] == -7.5 and (probs[1:] > 0).all() and sat.value > 0


def test_undefined_behaviour_of_the_reference_is_refused(case, bf):  # noqa: F811
    L = bf._lib.load()
    m, n = case.m, case.n_ids
    probs = np.full(n + 1, -7.5)
    sat = C.c_double(-1.0)

    def call(allowed_miss, n_bins):
        rc = L.btlbf_mibf_frame_probs(m._h, allowed_miss, C.c_void_p(probs.ctypes.data), n_bins, C.byref(sat))
        if rc:
            assert (probs == -7.5).all() and sat.value == -1.0  # nothing written
        return rc

    assert call(0, n - 1) == bf._lib.EINVAL and b"holds id" in L.btlbf_last_error()  # n at the largest id
    assert call(0, n - 2) == bf._lib.EINVAL                                           # ... and below it
    assert call(m.getHashNum() + 1, n) == bf._lib.EINVAL and b"allowed_miss" in L.btlbf_last_error()
    assert call(m.getHashNum(), n) == 0  # every miss allowed is defined
    probs[:] = -7.5
    sat.value = -1.0
    data = m.data()
    m.upload(np.zeros_like(data))  # no entry holds an id: sum == 0
    try:
        assert call(0, n) == bf._lib.EINVAL and b"no entry" in L.btlbf_last_error()
    finally:
        m.upload(data)
    assert call(0, n) == 0
