"""Classification of read pairs on the GPU (btlbf_mibf_classify_pairs, MIBloomFilter.classifyPairs) against the paired
model: tests/mibf_classify_model.py::classify over the two mates' frames interleaved, pinned to the reference's
query(itr1, itr2, minCount) by tests/test_mibf_classify_pairs_vs_ref.py.  Record for record, as check() of
tests/test_gpu_mibf_classify.py, including the zero rest of each row."""
import ctypes as C

import numpy as np
import pytest

import mibf_classify_model as cm
import mibf_model as mm
from test_gpu_mibf_classify import ACGT, Case, bf, long_case  # noqa: F401  (fixtures)
from test_mibf_classify_pairs_vs_ref import interleave, make_pairs
from test_mibf_classify_vs_ref import CFGS, K, LARGE, make_case, param_sets

pytestmark = pytest.mark.gpu
N = ord("N")


class PairCase(Case):
    """a miBF built on the GPU from the genomes of make_case(cfg, id_bytes), and the pairs of make_pairs on them"""

    def __init__(self, bf, cfg, id_bytes, bits=1 << 18):
        self.bf, self.id_bytes = bf, id_bytes
        self.seeds, self.h = CFGS[cfg]
        seqs, ids, _, _, _, self.prob, self.minc = make_case(cfg, id_bytes)
        self.genomes = [np.frombuffer(g, np.uint8) for g in seqs]
        seq = np.concatenate(self.genomes)
        starts = np.concatenate([[0], np.cumsum([g.size for g in self.genomes])]).astype(np.uint64)
        f = bf.BloomFilter(bits, self.h, K)
        if self.seeds:
            f.setSpacedSeeds(self.seeds, 1)
        f.insertSeqs(seq, starts=starts)
        self.ranks = mm.Ranks(f.download(), bits)
        self.m = bf.MIBloomFilter(f, id_bytes)
        f.close()
        self.m.insertIDs(seq, ids, starts=starts)
        self.m.insertSaturation(seq, ids, starts=starts, serial=True)
        self.data = self.m.data().astype(np.int64)
        self.n_ids = len(self.prob)
        self.pairs = [(np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)) for a, b in make_pairs(cfg, id_bytes)]


def model(case, pairs, p):
    ec, lim, mx, mc, agree = p
    return [cm.classify(case.data, case.ranks, interleave(case.rows(a), case.rows(b)), case.id_bytes, bool(case.seeds),
                        case.prob, case.minc, extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_count=mc,
                        best_hit_agree=bool(agree)) for a, b in pairs]


def gpu(case, pairs, p, max_results=8, read_len=0, device=False):
    ec, lim, mx, mc, agree = p
    seq, starts = case.bf.interleave_mates([a for a, _ in pairs], [b for _, b in pairs])
    if read_len:
        assert all(len(m) == read_len for pair in pairs for m in pair)
        starts = None
    if device:
        import torch

        seq = torch.from_numpy(seq.copy()).cuda()
        starts = None if read_len else torch.from_numpy(starts.astype(np.int64)).cuda()
    hits, n, sat, ev = case.m.classifyPairs(seq, case.prob, case.minc, extra_count=ec, extra_frame_limit=lim, max_miss=mx,
                                            min_frames=mc, best_hit_agree=bool(agree), max_results=max_results,
                                            starts=starts, read_len=read_len)
    if device:
        hits = case.bf.engine.hits_from_words(hits.cpu().numpy())
        n, sat, ev = (x.cpu().numpy().astype(np.uint32) for x in (n, sat, ev))
    return hits, n, sat, ev


def check(case, pairs, p, got, max_results=8):
    hits, n, sat, ev = got
    exp = model(case, pairs, p)
    assert len(n) == len(sat) == len(ev) == len(hits) == len(pairs)
    for i, (res, s, e) in enumerate(exp):
        assert (int(n[i]), int(sat[i]), int(ev[i])) == (len(res), s, e), (p, i)
        w = min(len(res), max_results)
        assert [tuple(int(x) for x in hits[i, j]) for j in range(w)] == [tuple(r) for r in res[:w]], (p, i)
        assert not hits[i, w:].view(np.uint8).any(), (p, i)  # the rest of the row is zero
    return exp


@pytest.fixture(scope="module")
def cases(bf):  # noqa: F811
    return {(c, b): PairCase(bf, c, b) for c in CFGS for b in (2, 4)}


@pytest.mark.parametrize("cfg", list(CFGS))
def test_parameter_grid_ragged_host(cases, cfg):
    """the whole grid of the reference pin, uint16 ids, the 20 pairs of the reference pin in host memory"""
    case = cases[cfg, 2]
    results = early = 0
    for p in param_sets(bool(case.seeds)):
        exp = check(case, case.pairs, p, gpu(case, case.pairs, p))
        results += sum(len(r[0]) >= 1 for r in exp)
        if p[1] != LARGE:  # the same set without the stop comes later in the grid; evalCount shows who stopped
            full = model(case, case.pairs, (p[0], LARGE) + p[2:])
            early += sum(a[2] < b[2] for a, b in zip(exp, full))
    assert results and early


@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_uint32_ids_fixed_layout_and_device(cases, cfg, device):
    """uint32 ids; a fixed read_len layout (mates padded with N to 120) and the ragged one; host and device inputs"""
    case = cases[cfg, 4]
    pad = lambda s: np.concatenate([s, np.full(120 - s.size, N, np.uint8)])
    padded = [(pad(a), pad(b)) for a, b in case.pairs]
    for p in param_sets(bool(case.seeds))[::5]:
        check(case, case.pairs, p, gpu(case, case.pairs, p, device=device))
        check(case, padded, p, gpu(case, padded, p, read_len=120, device=device))


def edge_pairs(case):
    """the smallest shapes at which the paired walk can go wrong, on genome 0 (350 bases) and its neighbours"""
    g, g1, g2 = case.genomes[0], case.genomes[1], case.genomes[2]
    ns = lambda n: np.full(n, N, np.uint8)
    gap = np.concatenate([g[:40], ns(100), g[150:190]])  # its second chunk (windows 64..127) has no clean window
    tail = np.concatenate([g[100:160], ns(90)])  # frames in its first chunk only; chunks 2 and 3 are all dirty
    none = np.zeros(0, np.uint8)
    return [
        (g[:40], g[150:350]),           # mates of 1 and 3 chunks
        (g[150:350], g[:40]),           # ... and of 3 and 1
        (np.concatenate([g, g1])[100:300], g2[:200]),  # 3 chunks each
        (gap, g[200:280]),              # a chunk without a clean window in mate 1
        (g[200:280], gap),              # ... in mate 2
        (gap, gap[::-1].copy()),        # ... in both
        (tail, g[150:350]),             # mate 1 exhausted while its range is not, mate 2 goes on alone
        (g[150:350], tail),             # ... mate 2
        (g[:K + 3], g[150:300]),        # mate 1 exhausted first
        (g[150:300], g[:K + 3]),        # mate 2 exhausted first
        (g[:K - 1], g[160:240]),        # a mate shorter than k
        (g[160:240], g[:K - 1]),
        (none, g[160:240]),             # an empty mate
        (g[160:240], none),
        (none, none),                   # both empty
        (ns(50), ns(70)),               # no frame in either
        (g[5:5 + K], g[160:240]),       # a single-frame mate
        (g[160:240], g[5:5 + K]),
        (g[5:5 + K], g1[7:7 + K]),      # two single frames
        (np.concatenate([g[:63 + K], ns(1)]), np.concatenate([ns(1), g[150:150 + 64 + K]])),  # frames end / begin at a chunk edge
    ]


@pytest.mark.parametrize("cfg", ["nt3", "C5"])
def test_chunk_and_exhaustion_edges(cases, cfg):
    case = cases[cfg, 2]
    pairs = edge_pairs(case)
    for p in [(1.0, 0, 0, 1, 0), (1.0, 2, 1 if case.seeds else 0, 1, 0), (2.0, LARGE, 0, 1, 1)]:
        exp = check(case, pairs, p, gpu(case, pairs, p))
        assert exp[14] == ([], 0, 0) and exp[15] == ([], 0, 0)
        assert exp[18][2] > 0  # the single frames were looked up
    # the order matters in these shapes: swapping the mates changes some result under the early stop
    p = (1.0, 0, 0, 1, 0)
    assert any(a != b for a, b in zip(model(case, pairs, p), model(case, [(b, a) for a, b in pairs], p)))


def test_a_lone_mate_equals_the_single_query(cases):
    """(s, empty) and (empty, s) are the single query of s"""
    case = cases["C5", 2]
    reads = [m for pair in case.pairs[:10] for m in pair]
    assert len(reads) == 20
    none = np.zeros(0, np.uint8)
    for p in [(1.0, 2, 1, 1, 0), (2.0, LARGE, 0, 3, 1)]:
        single = Case.gpu(case, reads, p)
        for pairs in ([(s, none) for s in reads], [(none, s) for s in reads]):
            got = gpu(case, pairs, p)
            for a, b in zip(single, got):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_batch_split_budget_and_empty_buffer(cases, bf):  # noqa: F811
    case = cases["C5", 2]
    p = (1.0, 2, 1, 1, 0)
    whole = gpu(case, case.pairs, p)
    check(case, case.pairs, p, whole)
    case.m.setScratchBudget(4096)  # a pair of two 120-base mates costs 240 * 10 + 128 bytes: one or two pairs per batch
    try:
        split = gpu(case, case.pairs, p)
    finally:
        case.m.setScratchBudget(0)
    for a, b in zip(whole, split):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    case.m.setScratchBudget(64)
    try:
        with pytest.raises(bf._lib.BtlbfError) as ei:
            gpu(case, case.pairs, p)
        assert ei.value.code == bf._lib.ENOMEM
    finally:
        case.m.setScratchBudget(0)
    hits, n, sat, ev = case.m.classifyPairs(np.zeros(0, np.uint8), case.prob, case.minc, read_len=100)
    assert len(n) == len(sat) == len(ev) == len(hits) == 0
    hits, n, sat, ev = case.m.classifyPairs(np.zeros(0, np.uint8), case.prob, case.minc, starts=np.zeros(1, np.uint64))
    assert len(n) == 0


def test_an_odd_number_of_sequences_is_refused(cases, bf):  # noqa: F811
    """EINVAL, and no byte of the four outputs is written; the same call with an even count goes through"""
    case = cases["nt3", 2]
    mates = [m for pair in case.pairs[:2] for m in pair]
    seq = np.concatenate(mates)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in mates])]).astype(np.uint64)
    hits = np.full((2, 2, 4), 0xABABABAB, np.uint32)
    outs = [np.full(2, 7, np.uint32) for _ in range(3)]
    L = bf._lib
    par = L.MibfClassifyParams(1.0, 0, 0, 1, 0, 2)
    prob = np.asarray(case.prob, np.float64)
    minc = np.asarray(case.minc, np.uint32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(lay, n_bytes):
        return L.load().btlbf_mibf_classify_pairs(case.m._h, ptr(seq), n_bytes, C.byref(lay), C.byref(par), ptr(prob),
                                                  ptr(minc), len(prob), ptr(hits), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                                  L.HOST, None)

    assert call(L.Layout(C.c_void_p(starts.ctypes.data), 3, 0), int(starts[3])) == L.EINVAL
    assert (hits == 0xABABABAB).all() and all((o == 7).all() for o in outs)
    assert call(L.Layout(None, 0, 40), 120) == L.EINVAL  # three sequences of a fixed length
    assert (hits == 0xABABABAB).all() and all((o == 7).all() for o in outs)
    assert call(L.Layout(C.c_void_p(starts.ctypes.data), 4, 0), seq.size) == 0
    assert not (hits == 0xABABABAB).any() and not any((o == 7).all() for o in outs[1:])
    with pytest.raises(bf._lib.BtlbfError) as ei:
        case.m.classifyPairs(seq[: int(starts[3])], case.prob, case.minc, starts=starts[:4])
    assert ei.value.code == L.EINVAL


def test_a_long_mate_takes_the_global_table(long_case):  # noqa: F811
    """a pair with a 5000-base mate over about 300 ids needs more slots than an LDS table holds; also when a budget puts
    it into a later batch than the small pair.  The small pair's table must hold the ids of BOTH mates: two mates of 46
    bases have at most 92 - 30 = 62 frames of 4 values, fewer than 256, and stay in LDS (two of 80 bases could meet all
    301 ids and would not).  The small pair costs 92 * 10 + 128 = 1048 bytes, the big one
    5080 * 10 + 128 + 512 * 24 + 12 = 63228, so 64000 bytes hold either but not both
    (tests/cpp/test_mibf_plan_pairs.cpp asserts that plan)."""
    case, contig = long_case
    assert case.n_ids == 301 and case.h == 4 and case.id_bytes == 2
    p = (1.0, LARGE, 1, 1, 0)
    pairs = [(contig[:80], contig[:5000]), (contig[100:146], contig[200:246])]

    def run(pairs):
        exp = [cm.classify(case.data, case.ranks, interleave(case.rows(a), case.rows(b)), 2, True, case.prob, case.minc,
                           extra_count=p[0], extra_frame_limit=p[1], max_miss=p[2], min_count=p[3]) for a, b in pairs]
        got = gpu(case, pairs, p)
        hits, n, sat, ev = got
        for i, (res, s, e) in enumerate(exp):
            assert (int(n[i]), int(sat[i]), int(ev[i])) == (len(res), s, e), i
            w = min(len(res), 8)
            assert [tuple(int(x) for x in hits[i, j]) for j in range(w)] == [tuple(r) for r in res[:w]], i
            assert not hits[i, w:].view(np.uint8).any(), i
        return got

    whole = run(pairs)
    assert case.m.classifyPaths() == (1, 1)
    swapped = run(pairs[::-1])
    case.m.setScratchBudget(64000)
    try:
        split = run(pairs[::-1])
        paths = case.m.classifyPaths()
    finally:
        case.m.setScratchBudget(0)
    assert paths == (1, 1)
    for a, b in zip(swapped, split):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    for a, b in zip(whole, swapped):
        assert np.asarray(a)[::-1].tobytes() == np.asarray(b).tobytes()
