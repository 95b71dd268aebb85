"""The read screen on the GPU (btlbf_screen_seqs / btlbf_screen_tally through screenSeqs / screen_tally), at the shapes
at which the fused kernel can go wrong.  hits[:, j] and valid are DEFINED as what containsSeqs on filter j followed by
count_per_seq returns (include/btlbf.h), so that path gives the expected values (screen_cases.existing_path); for the
ragged buffers the CPU oracle gives them a second time (bf_insert_seq / bf_contains_seq_dense per sequence, summed).

  ragged       lengths 0 .. 5000 across tile and workgroup-run boundaries, N runs, lowercase, an all-N sequence; k = 25 /
               h = 3 and k = 31 / h = 4; three filters of 2^16, 100000 and 2^32 + 2^20 + 64 bits (a bit filter's size is
               a multiple of 8, so 100000 stands for "a size of no power of two"), each holding a different third of the
               sequences; host and device buffers; no layout at all on one 5000-base sequence
  read_len     4099 reads of 150 (a tile of 2048 window starts is no whole number of reads); read_len 64 with k = 64
  spaced       two seeds of weight below k on every filter, the same ragged buffer
  counts       1, 2, 3, 4, 5, 8, 9, 16 filters over one buffer: column j depends neither on the number of filters nor on
               their order
  verdict      min_fraction x min_hits against numpy (screen_model); the tally against numpy: ties, accumulation, more
               rows than one launch's workgroups hold at a row per lane
  hashes       h = 5, 7, 8: the second wave of probes takes three values a step, so its loop runs two and three times
  contracts    poisoned and guarded outputs; a DEVICE call on a non-blocking stream whose inputs are still in flight;
               DEVICE calls on two streams in turn (the scratch they share); fresh and cleared filters; the filters'
               digests before and after"""
import numpy as np
import pytest

import poison
import screen_cases as sc
from poison import POISONS, assert_same
from screen_model import tally_model, verdict_model
from stream_gate import calibrate, run_gated
from test_gpu_auto_query import bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


class Case:
    """a ragged buffer, its three filters and both expectations"""

    def __init__(self, bf, oracle, k, h, seed):  # noqa: F811
        self.k, self.h = k, h
        self.r = sc.Ragged(k, seed)
        self.bodies = sc.oracle_bodies(oracle, self.r.seqs, sc.SIZES3, h, k)
        self.filters = sc.make_filters(bf, self.bodies, sc.SIZES3, h, k)
        self.exp = sc.existing_path(bf, self.filters, self.r.buf, k, starts=self.r.starts)
        self.oracle = sc.oracle_counts(oracle, self.r.seqs, self.bodies, sc.SIZES3, h, k)
        self.bodies = None  # (half a gigabyte)


@pytest.fixture(scope="module")
def cases(bf, oracle):  # noqa: F811
    return {(25, 3): Case(bf, oracle, 25, 3, 101), (31, 4): Case(bf, oracle, 31, 4, 102)}


def same(note, got, exp):
    hits, valid = sc.host(got[0]), sc.host(got[1])
    assert hits.shape == exp[0].shape and valid.shape == exp[1].shape, note
    bad = np.argwhere(hits != exp[0])
    assert bad.size == 0, "%s: hits differ at (row, filter) %s: %s, expected %s" % (
        note, bad[0].tolist(), hits[tuple(bad[0])], exp[0][tuple(bad[0])])
    bad = np.flatnonzero(valid != exp[1])
    assert bad.size == 0, "%s: valid differs at row %d: %d, expected %d" % (note, bad[0], valid[bad[0]], exp[1][bad[0]])


# ---------------------------------------------------------------------------------------------
# ragged layout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kh", [(25, 3), (31, 4)], ids=["k25h3", "k31h4"])
def test_the_two_expectations_agree_and_are_worth_testing(cases, kh):
    c = cases[kh]
    assert (c.exp[0] == c.oracle[0]).all() and (c.exp[1] == c.oracle[1]).all()
    hits, valid = c.exp
    frac = hits[valid > 0] / valid[valid > 0, None]
    for j in range(3):  # the columns differ; inserted sequences are found whole, the small filters give false positives
        assert (frac[:, j] == 1.0).sum() >= 10
    assert (hits[:, 0] != hits[:, 2]).any() and (hits[:, 1] != hits[:, 2]).any() and (hits[:, 0] != hits[:, 1]).any()
    assert ((frac[:, 0] > 0) & (frac[:, 0] < 1)).any() and ((frac[:, 1] > 0) & (frac[:, 1] < 1)).any()
    assert (valid == 0).sum() >= 12 and valid.max() >= 4900


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("kh", [(25, 3), (31, 4)], ids=["k25h3", "k31h4"])
def test_ragged(bf, cases, kh, mem):  # noqa: F811
    import torch

    c = cases[kh]
    buf, starts = c.r.buf, c.r.starts
    if mem == "device":
        buf, starts = torch.from_numpy(buf).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
    got = bf.screenSeqs(c.filters, buf, starts=starts)
    same("screenSeqs vs containsSeqs + count_per_seq", got, c.exp)
    same("screenSeqs vs the CPU oracle", got, c.oracle)
    assert (sc.host(got[2]) == verdict_model(c.exp[0], c.exp[1], 0.0, 1)).all()


@pytest.mark.parametrize("mem", ["host", "device"])
def test_no_layout_is_one_sequence(bf, cases, mem):  # noqa: F811
    import torch

    c = cases[(31, 4)]
    i = max(range(c.r.n), key=lambda q: c.r.seqs[q].size)
    s = c.r.seqs[i]
    assert s.size == 5000
    got = bf.screenSeqs(c.filters, torch.from_numpy(s).cuda() if mem == "device" else s)
    assert sc.host(got[0]).shape == (1, 3) and sc.host(got[1]).shape == (1,)
    same("one sequence, no layout", got, (c.exp[0][i:i + 1], c.exp[1][i:i + 1]))
    # ... and through the existing path given that sequence alone
    same("one sequence, no layout", got, sc.existing_path(bf, c.filters, s, 31, starts=np.array([0, 5000], np.uint64)))


# ---------------------------------------------------------------------------------------------
# fixed read length
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_fixed_read_len_150(bf, cases, mem):  # noqa: F811
    import torch

    c = cases[(31, 4)]
    n, L = 4099, 150
    rng = np.random.RandomState(7)
    reads = sc.random_bases(rng, n * L).reshape(n, L)
    src = c.r.buf[c.r.starts[np.argmax(np.diff(c.r.starts.astype(np.int64)))]:][:5000]  # a sequence of the case
    for q in range(0, n, 5):  # every fifth read is cut out of it: partly or wholly in one of the filters
        o = rng.randint(0, 5000 - L)
        reads[q] = src[o:o + L]
    reads[3, 40] = ord("N")
    buf = reads.reshape(-1)
    assert (2048 % L) != 0 and buf.size % 2048 != 0
    exp = sc.existing_path(bf, c.filters, buf, 31, read_len=L)
    assert exp[1].max() == L - 30 and (exp[0] > 0).any()
    got = bf.screenSeqs(c.filters, torch.from_numpy(buf).cuda() if mem == "device" else buf, read_len=L)
    same("4099 reads of 150", got, exp)


def test_read_len_equals_k_64(bf, oracle):  # noqa: F811
    k, h, n = 64, 3, 777
    rng = np.random.RandomState(8)
    reads = sc.random_bases(rng, n * k).reshape(n, k)
    reads[5, 63] = ord("N")
    reads[6, 0] = ord("n")
    sizes = (1 << 16, 100000)
    bodies = sc.oracle_bodies(oracle, [r for r in reads[: n // 2]], sizes, h, k)
    filters = sc.make_filters(bf, bodies, sizes, h, k)
    buf = reads.reshape(-1)
    exp = sc.existing_path(bf, filters, buf, k, read_len=k)
    assert exp[1].max() == 1 and exp[1][5] == 0 and exp[1][6] == 0 and exp[0][: n // 2].sum() >= n // 2 - 2
    same("read_len 64, k 64", bf.screenSeqs(filters, buf, read_len=k), exp)


# ---------------------------------------------------------------------------------------------
# more hash values than one step of the second wave takes (three): its loop runs twice for h = 5 and 7, a third time for 8
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("h", [5, 7, 8])
def test_more_hashes_than_one_step(bf, oracle, cases, h, mem):  # noqa: F811
    import torch

    r = cases[(31, 4)].r
    sizes = (1 << 16, 100000, 1 << 21)
    bodies = sc.oracle_bodies(oracle, r.seqs, sizes, h, 31)
    filters = sc.make_filters(bf, bodies, sizes, h, 31)
    exp = sc.existing_path(bf, filters, r.buf, 31, starts=r.starts)
    orc = sc.oracle_counts(oracle, r.seqs, bodies, sizes, h, 31)
    assert (exp[0] == orc[0]).all() and (exp[1] == orc[1]).all()
    frac = exp[0][exp[1] > 0] / exp[1][exp[1] > 0, None]
    # windows that survive every step (the inserted sequences) and windows that drop out on the way (the small filters'
    # false positives: few whole k-mers, so some probe after the first fails)
    assert (frac == 1.0).any(axis=0).all() and ((frac[:, 0] > 0) & (frac[:, 0] < 1)).any()
    buf, starts = r.buf, r.starts
    if mem == "device":
        buf, starts = torch.from_numpy(buf).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
    same("h = %d" % h, bf.screenSeqs(filters, buf, starts=starts), exp)


# ---------------------------------------------------------------------------------------------
# spaced seeds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device"])
def test_spaced_seeds(bf, cases, mem):  # noqa: F811
    import torch

    r = cases[(31, 4)].r
    filters = sc.make_filters(bf, [None] * 3, sc.SIZES3, len(sc.SEEDS2), 31, seeds=sc.SEEDS2)
    for j, f in enumerate(filters):  # a third of the sequences each, through the existing insert
        part = [s for i, s in enumerate(r.seqs) if i % 3 == j]
        f.insertSeqs(np.concatenate(part), starts=np.concatenate([[0], np.cumsum([s.size for s in part])]).astype(np.uint64))
    exp = sc.existing_path(bf, filters, r.buf, 31, starts=r.starts)
    assert (exp[0] == exp[1][:, None]).any(axis=1).sum() >= 30 and (exp[0][:, 0] != exp[0][:, 2]).any()
    buf, starts = r.buf, r.starts
    if mem == "device":
        buf, starts = torch.from_numpy(buf).cuda(), torch.from_numpy(starts.view(np.int64)).cuda()
    same("two spaced seeds", bf.screenSeqs(filters, buf, starts=starts), exp)


# ---------------------------------------------------------------------------------------------
# the number of filters and their order
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sixteen(bf, oracle, cases):  # noqa: F811
    r = cases[(31, 4)].r
    sizes = tuple((1 << (14 + j % 5)) if j % 2 == 0 else 8 * (5000 + 37 * j) for j in range(16))
    bodies = sc.oracle_bodies(oracle, r.seqs, sizes, 4, 31)
    filters = sc.make_filters(bf, bodies, sizes, 4, 31)
    return r, filters, sc.existing_path(bf, filters, r.buf, 31, starts=r.starts)


@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8, 9, 16])
def test_filter_counts_and_order(bf, sixteen, nf):  # noqa: F811
    r, filters, exp = sixteen
    got = bf.screenSeqs(filters[:nf], r.buf, starts=r.starts)
    same("%d filters" % nf, got, (exp[0][:, :nf], exp[1]))
    perm = np.random.RandomState(nf).permutation(16)[:nf]  # any nf of the sixteen, in any order
    got = bf.screenSeqs([filters[p] for p in perm], r.buf, starts=r.starts)
    same("%d filters, permuted" % nf, got, (exp[0][:, perm], exp[1]))
    assert len({exp[0][:, j].tobytes() for j in range(16)}) == 16  # no two columns alike: a swap would show


# ---------------------------------------------------------------------------------------------
# verdict and tally
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_hits", [0, 1, 5])
@pytest.mark.parametrize("min_fraction", [0.0, 0.15, 0.5, 1.0])
def test_verdict_and_tally(bf, cases, min_fraction, min_hits):  # noqa: F811
    c = cases[(31, 4)]
    hits, valid, pb = bf.screenSeqs(c.filters, c.r.buf, starts=c.r.starts, min_fraction=min_fraction, min_hits=min_hits)
    exp_pb = verdict_model(c.exp[0], c.exp[1], min_fraction, min_hits)
    assert (pb == exp_pb).all(), np.flatnonzero(pb != exp_pb)
    assert (pb[valid == 0] == 0).all() and (valid == 0).any()  # a row without a clean window never passes
    if min_fraction in (0.15, 0.5):
        assert 0 < (pb != 0).sum() < len(pb)
    passed, best, totals = bf.screen_tally(hits, valid, pb)
    exp = tally_model(hits, valid, pb)
    assert [x.tolist() for x in (passed, best, totals)] == [x.tolist() for x in exp]
    # a second call adds to the first
    passed2, best2, totals2 = bf.screen_tally(hits, valid, pb, passed=passed.copy(), best=best.copy(), totals=totals.copy())
    assert [x.tolist() for x in (passed2, best2, totals2)] == [(2 * x).tolist() for x in exp]


def test_tally_ties_go_to_the_lowest_index(bf):  # noqa: F811
    hits = np.array([[4, 4, 4, 4], [1, 9, 9, 2], [0, 3, 3, 3], [7, 7, 1, 7], [5, 5, 5, 5], [2, 2, 2, 9]], np.uint32)
    valid = np.array([10, 10, 10, 10, 0, 10], np.uint32)
    pb = np.array([0b1111, 0b1110, 0b1100, 0b1001, 0, 0b0111], np.uint32)  # (bits as given: not recomputed by the tally)
    passed, best, totals = bf.screen_tally(hits, valid, pb)
    assert best.tolist() == [3, 1, 1, 0]  # rows 0, 3, 5 -> 0 (row 5: filter 3 does not pass); row 1 -> 1; row 2 -> 2
    assert passed.tolist() == [3, 3, 4, 4] and totals.tolist() == [6, 1, 5, 1]
    assert [x.tolist() for x in tally_model(hits, valid, pb)] == [passed.tolist(), best.tolist(), totals.tolist()]


def test_verdict_and_tally_on_a_case_worked_by_hand(bf):  # noqa: F811
    """the numpy model and the library on rows small enough to check by eye: float64, one multiply, one >=; rows without
    a clean window never pass; ties to the lowest index"""
    hits = np.array([[3, 3, 0], [0, 0, 0], [5, 9, 9], [1, 0, 0], [2, 7, 1]], np.uint32)
    valid = np.array([6, 0, 10, 120, 7], np.uint32)
    pb = verdict_model(hits, valid, 0.5, 1)
    assert pb.tolist() == [0b011, 0, 0b111, 0, 0b010]
    assert verdict_model(hits, valid, 0.0, 0).tolist() == [0b111, 0, 0b111, 0b111, 0b111]
    passed, best, totals = bf.screen_tally(hits, valid, pb)
    assert passed.tolist() == [2, 3, 1] and best.tolist() == [1, 2, 0] and totals.tolist() == [5, 2, 2, 1]
    assert [x.tolist() for x in tally_model(hits, valid, pb)] == [passed.tolist(), best.tolist(), totals.tolist()]


def test_device_calls_on_two_streams_share_the_scratch_in_order(bf, cases):  # noqa: F811
    """a DEVICE call returns with its work queued; the bitmaps it reduces are one filter's scratch, which the next call
    -- here on another stream, with another buffer -- may only take over when the first has run"""
    import torch

    c = cases[(31, 4)]
    big = torch.from_numpy(np.tile(c.r.buf[: 150 * 300], 40)).cuda()  # 12000 reads of 150
    exp_big = sc.existing_path(bf, c.filters, big.cpu().numpy(), 31, read_len=150)
    rag, st = torch.from_numpy(c.r.buf).cuda(), torch.from_numpy(c.r.starts.view(np.int64)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            outs.append(("big", bf.screenSeqs(c.filters, big, read_len=150)))
        with torch.cuda.stream(s2):
            outs.append(("ragged", bf.screenSeqs(c.filters, rag, starts=st)))
    torch.cuda.synchronize()
    for name, got in outs:
        same(name, got, exp_big if name == "big" else c.exp)


def test_tally_of_more_rows_than_one_pass_of_the_grid(bf):  # noqa: F811
    """512 workgroups of 256 lanes take 131072 rows per pass; device arrays, device totals, twice"""
    import torch

    n, nf = 140001, 5
    rng = np.random.RandomState(11)
    hits = rng.randint(0, 6, (n, nf)).astype(np.uint32)  # few distinct values: many ties
    valid = rng.randint(0, 4, n).astype(np.uint32)
    pb = rng.randint(0, 1 << nf, n).astype(np.uint32)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    d = (dev(hits), dev(valid), dev(pb))
    passed, best, totals = bf.screen_tally(*d)
    passed, best, totals = bf.screen_tally(*d, passed=passed, best=best, totals=totals)
    exp = tally_model(hits, valid, pb)
    assert [x.cpu().numpy().tolist() for x in (passed, best, totals)] == [(2 * x).tolist() for x in exp]
    assert totals[0].item() == 2 * n


# ---------------------------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", POISONS)
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("layout", ["ragged", "read_len", "none"])
def test_every_output_element_is_written_and_nothing_else(bf, cases, monkeypatch, byte, mem, layout):  # noqa: F811
    import torch

    c = cases[(31, 4)]
    if layout == "ragged":
        buf, kw, exp = c.r.buf, dict(starts=c.r.starts), c.exp
    elif layout == "read_len":
        buf = c.r.buf[: 150 * 61]
        kw = dict(read_len=150)
        exp = sc.existing_path(bf, c.filters, buf, 31, read_len=150)
    else:
        buf, kw = c.r.buf[:3001], {}
        exp = sc.existing_path(bf, c.filters, buf, 31, starts=np.array([0, 3001], np.uint64))
    exp_pb = verdict_model(exp[0], exp[1], 0.5, 2)
    if mem == "device":
        buf = torch.from_numpy(buf).cuda()
        kw = {k: (torch.from_numpy(v.view(np.int64)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    poison.poisoned_outputs(monkeypatch, byte)
    hits, valid, pb = bf.screenSeqs(c.filters, buf, min_fraction=0.5, min_hits=2, **kw)
    assert_same("hits", hits, exp[0])
    assert_same("valid", valid, exp[1])
    assert_same("pass_bits", pb, exp_pb)
    poison.check_guards()


@pytest.fixture(scope="module")
def delay(bf):  # noqa: F811
    return calibrate()


@pytest.mark.parametrize("byte", POISONS)
def test_device_call_on_a_non_blocking_stream_with_late_inputs(bf, cases, delay, monkeypatch, byte):  # noqa: F811
    """the sequence bytes and the device `starts` arrive on the stream after the call was issued; until then the buffers
    hold another valid input of the same size"""
    c = cases[(31, 4)]
    lens = np.diff(c.r.starts.astype(np.int64))
    decoy_starts = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.uint64)
    decoy_buf = c.r.buf[::-1].copy()
    assert (decoy_starts != c.r.starts).any() and decoy_starts[-1] == c.r.starts[-1]
    exp_pb = verdict_model(c.exp[0], c.exp[1], 0.15, 1)

    def setup(g):
        seq = g.late(None, c.r.buf, decoy_buf)
        st = g.late(None, c.r.starts, decoy_starts)
        return lambda: bf.screenSeqs(c.filters, seq, starts=st, min_fraction=0.15)

    def check(got, note):
        assert_same(note + ": hits", got[0], c.exp[0])
        assert_same(note + ": valid", got[1], c.exp[1])
        assert_same(note + ": pass_bits", got[2], exp_pb)

    run_gated("screenSeqs", delay, setup, check, monkeypatch, byte)


def test_fresh_and_cleared_filters_give_zero_columns(bf, cases):  # noqa: F811
    c = cases[(31, 4)]
    fresh = bf.BloomFilter(1 << 20, 4, 31)
    cleared = bf.BloomFilter(100000, 4, 31)
    cleared.insertSeqs(c.r.buf, starts=c.r.starts)
    full = bf.screenSeqs([cleared], c.r.buf, starts=c.r.starts)
    assert (full[0][:, 0] == c.exp[1]).all() and c.exp[1].sum() > 40000  # everything it was given
    cleared.clear()
    hits, valid, pb = bf.screenSeqs([fresh, c.filters[0], cleared], c.r.buf, starts=c.r.starts)
    assert (hits[:, 0] == 0).all() and (hits[:, 2] == 0).all() and (hits[:, 1] == c.exp[0][:, 0]).all()
    assert (valid == c.exp[1]).all() and ((pb & 0b101) == 0).all()
    assert fresh.getPop() == 0 and cleared.getPop() == 0


def test_the_filters_are_not_changed(bf, cases, sixteen):  # noqa: F811
    c = cases[(31, 4)]
    _, filters, _ = sixteen
    for fs in (c.filters, filters):
        before = [f.digest() for f in fs]
        bf.screenSeqs(fs, c.r.buf, starts=c.r.starts)
        assert [f.digest() for f in fs] == before
