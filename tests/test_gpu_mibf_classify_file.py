"""Read classification from FASTQ files (btlbf_mibf_classify_fastx_*, MIBloomFilter.classifyFile) against the same
reads classified from memory (classify / classifyPairs, themselves pinned to the model and the reference by
tests/test_gpu_mibf_classify*.py): row for row, in all four arrays, for single reads, two files, an interleaved file and
gzip input; with batches of a few reads, so that the two files' byte-cut batches hold different record counts (the
zipper of csrc/mibf_zip.hpp), and once with batches of exactly the longest read.  The summary equals the numpy model of
btlbf_mibf_classify_tally over all rows.

The reads are the queries of make_case and the pairs of make_pairs; the goldens of the reference pins assert on the
reference's own output that among them at least a third have a result, one has two, one has satCount > 0 and some have
no frame.  The same is asserted here on the in-memory result, over the two parameter sets used."""
import gzip

import numpy as np
import pytest

from mibf_tally_model import tally_model
from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)
from test_gpu_mibf_classify_pairs import PairCase
from test_mibf_classify_vs_ref import CFGS, LARGE, make_case, optimal_size, param_sets

pytestmark = pytest.mark.gpu
# (extra_count, extra_frame_limit, max_miss, min_count, agree): two sets of the reference pins' grid
PARAMS = [(1.0, 2, 1, 1, 0), (0.5, LARGE, 0, 1, 0)]
assert all(p in param_sets(True) for p in PARAMS)
MAX_RESULTS = 3


def kw(p):
    return dict(extra_count=p[0], extra_frame_limit=p[1], max_miss=p[2], min_frames=p[3], best_hit_agree=bool(p[4]),
                max_results=MAX_RESULTS)


def fastq(path, reads, first=0, gz=False):
    text = b"".join(b"@r%d comment\n%s\n+\n%s\n" % (first + i, bytes(s), b"I" * len(s)) for i, s in enumerate(reads))
    with (gzip.open if gz else open)(str(path), "wb") as f:
        f.write(text)
    return str(path)


class Files:
    def __init__(self, bf, tmp):
        # the miBF of the reference pins: their size, so that their conditions on these reads hold here as well
        _, _, entries, occupancy, _, _, _ = make_case("C5", 2)
        self.case = c = PairCase(bf, "C5", 2, bits=optimal_size(entries, CFGS["C5"][1], occupancy))
        self.reads = [np.frombuffer(s, np.uint8) for s in make_case("C5", 2)[4]]
        self.m1, self.m2 = [a for a, _ in c.pairs], [b for _, b in c.pairs]
        self.inter = [m for pair in c.pairs for m in pair]
        self.single = fastq(tmp / "single.fq", self.reads)
        self.f1, self.f2 = fastq(tmp / "r1.fq", self.m1), fastq(tmp / "r2.fq", self.m2)
        self.il = fastq(tmp / "il.fq", self.inter)
        self.mem = {}
        for p in PARAMS:
            seq = np.concatenate(self.reads)
            starts = np.concatenate([[0], np.cumsum([r.size for r in self.reads])]).astype(np.uint64)
            self.mem["single", p] = c.m.classify(seq, c.prob, c.minc, starts=starts, **kw(p))
            seq, starts = bf.interleave_mates(self.m1, self.m2)
            self.mem["pairs", p] = c.m.classifyPairs(seq, c.prob, c.minc, starts=starts, **kw(p))

    def paths(self, kind, gz_dir=None):
        """classifyFile's path arguments for a kind of input; gz_dir: the same input gzip-compressed, written there"""
        if kind == "single":
            args, reads = dict(path=self.single), dict(path=self.reads)
        elif kind == "two":
            args, reads = dict(path=self.f1, path2=self.f2), dict(path=self.m1, path2=self.m2)
        else:
            args, reads = dict(path=self.il, interleaved=True), dict(path=self.inter)
        if gz_dir is not None:
            for key, r in reads.items():
                args[key] = fastq(gz_dir / (key + ".fq.gz"), r, gz=True)
        return args

    def run(self, kind, p, batch_bytes, gz_dir=None, **more):
        c = self.case
        args = self.paths(kind, gz_dir)
        return c.m.classifyFile(args.pop("path"), c.prob, c.minc, batch_bytes=batch_bytes, **args, **more, **kw(p))


@pytest.fixture(scope="module")
def files(bf, tmp_path_factory):  # noqa: F811
    return Files(bf, tmp_path_factory.mktemp("fq"))


def collect(it, exp, n_batches_min=1):
    """the batches of a classifyFile iterator against the in-memory result; -> rows seen"""
    row = batches = 0
    for first, hits, n, sat, ev in it:
        assert first == row and len(hits) == len(n) == len(sat) == len(ev) > 0
        e = [np.asarray(x)[row:row + len(n)] for x in exp]
        assert hits.tobytes() == e[0].tobytes() and hits.dtype == e[0].dtype
        for g, x in zip((n, sat, ev), e[1:]):
            assert g.dtype == np.uint32 and g.tolist() == x.tolist()
        row += len(n)
        batches += 1
    assert batches >= n_batches_min
    return row


def test_the_comparison_is_not_vacuous(files):
    """the conditions the reference pins assert on the reference's output, here on the in-memory results"""
    for kind, n_rows in (("single", 24), ("pairs", 20)):
        two = sat_rows = 0
        for p in PARAMS:
            hits, n, sat, ev = files.mem[kind, p]
            assert len(n) == n_rows and 3 * (n >= 1).sum() >= n_rows, (kind, p)
            two += (n >= 2).sum()
            sat_rows += (sat > 0).sum()
            print(kind, p, "with result", (n >= 1).sum(), "two", (n >= 2).sum(), "sat", (sat > 0).sum(), "no frame",
                  (ev == 0).sum(), "truncated", (n > MAX_RESULTS).sum())
            if kind == "pairs":  # (short, read), (read, empty), (empty, empty), (all N, one frame)
                assert (ev == 0).sum() >= 1 and ev[16] > 0 and ev[17] > 0 and ev[18] == 0 and n[18] == 0
        assert two >= 1 and sat_rows >= 1, kind
    assert max(r.size for r in files.reads) <= 120 and max(m.size for m in files.inter) <= 120
    assert any(m.size == 0 for m in files.m1) and any(m.size == 0 for m in files.m2)


@pytest.mark.parametrize("kind", ["single", "two", "interleaved"])
@pytest.mark.parametrize("p", PARAMS, ids=["lim2_mm1", "lim_large_mm0"])
def test_rows_equal_the_in_memory_result(files, kind, p):
    exp = files.mem["single" if kind == "single" else "pairs", p]
    n_rows = len(exp[1])
    # ~400 bases per batch: at least five batches; the two files' batches then end at different records
    it = files.run(kind, p, 400)
    assert collect(it, exp, 5) == n_rows
    # the handle's running tally after the last batch, and the whole-file call, equal the model over all rows
    model = tally_model(*exp, files.case.n_ids, MAX_RESULTS)
    for got in (it.tally(), files.run(kind, p, 400, summary_only=True)):
        for g, e in zip(got, model):
            assert g.dtype == np.uint64 and g.tolist() == e.tolist()
    it.close()
    assert model[2][0] == n_rows and model[0].sum() == (exp[1] >= 1).sum()


@pytest.mark.parametrize("kind", ["single", "two", "interleaved"])
def test_batches_of_exactly_the_longest_read_and_one_batch(files, kind):
    p = PARAMS[0]
    exp = files.mem["single" if kind == "single" else "pairs", p]
    longest = max(r.size for r in (files.reads if kind == "single" else files.inter))
    assert collect(files.run(kind, p, longest), exp, 10) == len(exp[1])
    assert collect(files.run(kind, p, 0), exp, 1) == len(exp[1])  # the default batch: everything at once


def plan_cost(n, pair, k, h, id_bytes, n_ids):
    """what a read, or a pair, of n bytes takes of the scratch budget: the cost of mibf_plan_classify / _pairs
    (csrc/mibf_plan.hpp), the table of mibf_classify_cap slots included where it does not fit LDS"""
    cap = 16
    while cap <= min(max(n - k + 1, 0) * h, n_ids):
        cap <<= 1
    slots = cap if cap > 256 else 0
    return n * (h * id_bytes + 2) + (128 if pair else 64) + slots * 24 + (12 if slots else 0)


@pytest.mark.parametrize("kind", ["single", "two", "interleaved"])
def test_a_file_batch_cut_into_plan_batches(files, kind):
    """the whole file as one file batch under a scratch budget of 4096 bytes: the plan cuts it into at least four
    batches, whose offsets are rebased and staged by the handle's scratch; rows and tally as under the default budget"""
    c, p, budget = files.case, PARAMS[0], 4096
    exp = files.mem["single" if kind == "single" else "pairs", p]
    units = [r.size for r in files.reads] if kind == "single" else [a.size + b.size for a, b in c.pairs]
    costs = [plan_cost(n, kind != "single", len(c.seeds[0]), c.h, c.id_bytes, c.n_ids) for n in units]
    print(kind, "units", len(costs), "largest", max(costs), "sum", sum(costs))
    assert max(costs) <= budget and sum(costs) >= 4 * budget  # every unit fits; four batches at the least
    c.m.setScratchBudget(budget)
    try:
        it = files.run(kind, p, 0)
        batches = list(it)
        got = it.tally()
        it.close()
    finally:
        c.m.setScratchBudget(0)
    assert len(batches) == 1 and collect(iter(batches), exp) == len(exp[1]) == len(units)
    for g, e in zip(got, tally_model(*exp, c.n_ids, MAX_RESULTS)):
        assert g.dtype == np.uint64 and g.tolist() == e.tolist()


@pytest.mark.parametrize("kind", ["single", "two", "interleaved"])
def test_gzip_input(files, kind, tmp_path):
    p = PARAMS[1]
    exp = files.mem["single" if kind == "single" else "pairs", p]
    assert collect(files.run(kind, p, 400, gz_dir=tmp_path), exp, 5) == len(exp[1])


def test_a_mate_file_one_record_short(files, bf, tmp_path):  # noqa: F811
    """EFORMAT from the call that reaches the end; every pair that exists was delivered before, and equals"""
    c, p = files.case, PARAMS[0]
    exp = files.mem["pairs", p]
    for short in (1, 2):
        f1 = files.f1 if short == 2 else fastq(tmp_path / "s1.fq", files.m1[:-1])
        f2 = files.f2 if short == 1 else fastq(tmp_path / "s2.fq", files.m2[:-1])
        it = c.m.classifyFile(f1, c.prob, c.minc, path2=f2, batch_bytes=300, **kw(p))
        with pytest.raises(bf._lib.BtlbfError) as ei:
            collect(it, [np.asarray(x)[:19] for x in exp])
        assert ei.value.code == bf._lib.EFORMAT and "pair up" in str(ei.value)
        assert it.tally()[2][0] == 19
        it.close()
        with pytest.raises(bf._lib.BtlbfError) as ei:
            c.m.classifyFile(f1, c.prob, c.minc, path2=f2, batch_bytes=300, summary_only=True, **kw(p))
        assert ei.value.code == bf._lib.EFORMAT


def test_an_odd_interleaved_file(files, bf, tmp_path):  # noqa: F811
    c, p = files.case, PARAMS[0]
    exp = files.mem["pairs", p]
    path = fastq(tmp_path / "odd.fq", files.inter[:-1])
    it = c.m.classifyFile(path, c.prob, c.minc, interleaved=True, batch_bytes=300, **kw(p))
    with pytest.raises(bf._lib.BtlbfError) as ei:
        collect(it, [np.asarray(x)[:19] for x in exp])
    assert ei.value.code == bf._lib.EFORMAT and "no mate" in str(ei.value) and it.tally()[2][0] == 19


def test_a_record_longer_than_a_batch(files, bf):  # noqa: F811
    c, p = files.case, PARAMS[0]
    sizes = [r.size for r in files.reads]
    longest = max(sizes)
    it = c.m.classifyFile(files.single, c.prob, c.minc, batch_bytes=longest - 1, **kw(p))
    with pytest.raises(bf._lib.BtlbfError) as ei:
        list(it)
    assert ei.value.code == bf._lib.EINVAL and "record %d " % (sizes.index(longest) + 1) in str(ei.value)


def test_a_file_without_records_and_both_pairing_modes(files, bf, tmp_path):  # noqa: F811
    c, p = files.case, PARAMS[0]
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    it = c.m.classifyFile(str(empty), c.prob, c.minc, **kw(p))
    assert list(it) == [] and all(not x.any() for x in it.tally())
    best, any_, totals = c.m.classifyFile(str(empty), c.prob, c.minc, path2=str(empty), summary_only=True, **kw(p))
    assert not best.any() and not any_.any() and not totals.any() and len(best) == c.n_ids
    with pytest.raises(bf._lib.BtlbfError) as ei:
        c.m.classifyFile(files.f1, c.prob, c.minc, path2=files.f2, interleaved=True, **kw(p))
    assert ei.value.code == bf._lib.EINVAL
    with pytest.raises(bf._lib.BtlbfError) as ei:
        c.m.classifyFile(str(tmp_path / "missing.fq"), c.prob, c.minc, **kw(p))
    assert ei.value.code == bf._lib.EIO


def test_what_classify_reports_comes_back_unchanged(files, bf):  # noqa: F811
    """tables shorter than the ids of the array: EINVAL from the first batch; a read beyond the scratch budget: ENOMEM;
    more ids than the id type holds: EINVAL at open"""
    c, p = files.case, PARAMS[0]
    with pytest.raises(bf._lib.BtlbfError) as ei:
        list(c.m.classifyFile(files.single, c.prob[:5], c.minc[:5], **kw(p)))
    assert ei.value.code == bf._lib.EINVAL and "holds id" in str(ei.value)
    c.m.setScratchBudget(64)
    try:
        with pytest.raises(bf._lib.BtlbfError) as ei:
            c.m.classifyFile(files.f1, c.prob, c.minc, path2=files.f2, summary_only=True, **kw(p))
        assert ei.value.code == bf._lib.ENOMEM
    finally:
        c.m.setScratchBudget(0)
    with pytest.raises(bf._lib.BtlbfError) as ei:
        c.m.classifyFile(files.single, [0.001] * 32769, [1] * 32769, **kw(p))
    assert ei.value.code == bf._lib.EINVAL and "n_ids" in str(ei.value)
    assert collect(files.run("single", p, 400), files.mem["single", p], 5) == 24  # the miBF is as it was
