"""btlbf_mibf_classify_tally (classify_tally) against tests/mibf_tally_model.py over synthetic result arrays: 0, 1 and 257
rows (more than one workgroup of 256); n_ids = 3 with every row on one id (contention on one bin); n_ids = 8193 (one past
the workgroup bins in LDS: global atomics); max_results = 1 with rows of n_hits = 2 (truncated rows, `any` stops at
max_results); two calls into the same arrays add up; device and host memory."""
import numpy as np
import pytest

from mibf_tally_model import tally_model
from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def results(bf, n_rows, max_results, n_ids, seed, one_id=None, n_hits_of=None):
    rng = np.random.RandomState(seed)
    hits = np.zeros((n_rows, max_results), bf.engine.HIT_DTYPE)
    hits["id"] = rng.randint(0, n_ids, (n_rows, max_results)) if one_id is None else one_id
    if n_ids > 8192 and n_rows:
        hits["id"][0, 0] = n_ids - 1  # the last bin is used
    hits["count"] = rng.randint(0, 1 << 16, (n_rows, max_results))
    n_hits = rng.randint(0, max_results + 3, n_rows).astype(np.uint32) if n_hits_of is None else \
        np.full(n_rows, n_hits_of, np.uint32)
    sat = rng.randint(0, 1 << 31, n_rows).astype(np.uint32) * 2  # sums pass 2^32
    ev = rng.randint(0, 1000, n_rows).astype(np.uint32)
    return hits, n_hits, sat, ev


def same(got, exp):
    for g, e in zip(got, exp):
        assert np.asarray(g).astype(np.uint64).tolist() == e.tolist()


@pytest.mark.parametrize("n_rows", [0, 1, 257])
@pytest.mark.parametrize("n_ids,one_id", [(3, 2), (40, None), (8192, None), (8193, None)])
def test_against_numpy_host_and_device(bf, n_rows, n_ids, one_id):  # noqa: F811
    import torch

    r = results(bf, n_rows, 4, n_ids, n_rows + n_ids, one_id)
    exp = tally_model(*r, n_ids)
    if n_rows == 257:
        assert exp[2][4] > 1 << 32 and exp[2][1] and exp[2][2] and exp[2][3]
        assert exp[0][2] == exp[2][0] - exp[2][1] if one_id is not None else exp[0].max() >= 1
    same(bf.classify_tally(*r, n_ids), exp)
    dev = [torch.from_numpy(np.ascontiguousarray(r[0]).view(np.int32).reshape(n_rows, 4, 4)).cuda()] + \
        [torch.from_numpy(x.view(np.int32)).cuda() for x in r[1:]]
    got = bf.classify_tally(*dev, n_ids)
    torch.cuda.synchronize()
    same([g.cpu().numpy().view(np.uint64) for g in got], exp)


def test_truncated_rows_and_accumulation(bf):  # noqa: F811
    n_ids = 5
    a = results(bf, 257, 1, n_ids, 1, n_hits_of=2)  # two results each, one record kept
    ea = tally_model(*a, n_ids)
    assert ea[2].tolist()[:4] == [257, 0, 257, 257] and ea[1].sum() == 257 and (ea[0] == ea[1]).all()
    got = bf.classify_tally(*a, n_ids)
    same(got, ea)
    b = results(bf, 100, 1, n_ids, 2)
    eb = tally_model(*b, n_ids)
    got = bf.classify_tally(*b, n_ids, best=got[0], any_=got[1], totals=got[2])  # into the same arrays
    same(got, [x + y for x, y in zip(ea, eb)])


def test_an_id_beyond_the_bins_is_ignored(bf):  # noqa: F811
    hits, n_hits, sat, ev = results(bf, 10, 2, 4, 3, n_hits_of=2)
    hits["id"][3] = (4, 1 << 20)  # neither can come out of classify with n_ids = 4
    exp = tally_model(hits, n_hits, sat, ev, 4)
    assert exp[1].sum() == 18
    same(bf.classify_tally(hits, n_hits, sat, ev, 4), exp)
