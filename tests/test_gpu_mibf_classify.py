"""Read classification on the GPU (btlbf_mibf_classify_seqs, MIBloomFilter.classify) against the model of
tests/mibf_classify_model.py (pinned to the reference by tests/test_mibf_classify_vs_ref.py), record for record."""
import numpy as np
import pytest

import mibf_classify_model as cm
import mibf_model as mm
from test_mibf_classify_vs_ref import C5_SEEDS, CFGS, K, LARGE, param_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    return m


ACGT = np.frombuffer(b"ACGT", np.uint8)


def genomes_of(rng, n_ids, length=350, share=2):
    """every ID has a part of its own and, from 300 bases on, a part it shares with its share - 1 neighbours
    (saturation, reads that hit several IDs)"""
    if length < 300:
        return [ACGT[rng.randint(0, 4, length)] for _ in range(n_ids)]
    shared = [ACGT[rng.randint(0, 4, 110)] for _ in range((n_ids + share - 1) // share)]
    return [np.concatenate([ACGT[rng.randint(0, 4, 150)], shared[i // share], ACGT[rng.randint(0, 4, length - 260)]])
            for i in range(n_ids)]


class Case:
    """a miBF built on the GPU from n_ids related genomes (IDs 1..n_ids), its model state, and reads of them"""

    def __init__(self, bf, cfg, id_bytes, n_ids, n_reads=64, lo=40, hi=121, bits=1 << 18, seed=5, length=350, share=2):
        self.bf, self.id_bytes = bf, id_bytes
        self.seeds, self.h = CFGS[cfg]
        rng = np.random.RandomState(seed)
        gs = genomes_of(rng, n_ids, length, share)
        seq = np.concatenate(gs)
        starts = np.concatenate([[0], np.cumsum([g.size for g in gs])]).astype(np.uint64)
        f = bf.BloomFilter(bits, self.h, K)
        if self.seeds:
            f.setSpacedSeeds(self.seeds, 1)
        f.insertSeqs(seq, starts=starts)
        self.ranks = mm.Ranks(f.download(), bits)
        self.m = bf.MIBloomFilter(f, id_bytes)
        f.close()
        ids = np.arange(1, n_ids + 1)
        self.m.insertIDs(seq, ids, starts=starts)
        self.m.insertSaturation(seq, ids, starts=starts, serial=True)
        self.data = self.m.data().astype(np.int64)
        self.n_ids = n_ids + 1
        self.prob = [0.001 * (i + 1) for i in range(self.n_ids)]
        self.minc = [1 + i % 3 for i in range(self.n_ids)]
        reads = []
        for r in range(n_reads):
            g = gs[rng.randint(0, n_ids)]
            n = rng.randint(lo, hi)
            o = rng.randint(0, g.size - n + 1)
            s = g[o:o + n].copy()
            if r % 4 == 0:
                s[rng.randint(0, n)] = ord("N")
            reads.append(s)
        self.reads = reads

    def rows(self, s):
        s = np.ascontiguousarray(s, np.uint8)
        if s.size == 0:
            return np.zeros((0, self.h), np.uint64)
        if self.seeds:
            hv, valid, _ = self.bf.sthash_seqs(s, self.seeds, 1, K)
        else:
            hv, valid = self.bf.hash_seqs(s, self.h, K)
        return np.asarray(hv)[: s.size].astype(np.uint64)[self.bf.bits_to_bool(valid, s.size)]

    def model(self, reads, p):
        ec, lim, mx, mc, agree = p
        return [cm.classify(self.data, self.ranks, self.rows(s), self.id_bytes, bool(self.seeds), self.prob, self.minc,
                            extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_count=mc, best_hit_agree=bool(agree))
                for s in reads]

    def gpu(self, reads, p, max_results=8, read_len=0, device=False):
        ec, lim, mx, mc, agree = p
        seq = np.concatenate(reads) if len(reads) else np.zeros(0, np.uint8)
        starts = None if read_len else np.concatenate([[0], np.cumsum([len(s) for s in reads])]).astype(np.uint64)
        if device:
            import torch

            seq = torch.from_numpy(seq).cuda()
            starts = None if read_len else torch.from_numpy(starts.astype(np.int64)).cuda()
        hits, n, sat, ev = self.m.classify(seq, self.prob, self.minc, extra_count=ec, extra_frame_limit=lim, max_miss=mx,
                                           min_frames=mc, best_hit_agree=bool(agree), max_results=max_results,
                                           starts=starts, read_len=read_len)
        if device:
            hits = self.bf.engine.hits_from_words(hits.cpu().numpy())
            n, sat, ev = (x.cpu().numpy().astype(np.uint32) for x in (n, sat, ev))
        return hits, n, sat, ev


def check(case, reads, p, got, max_results=8):
    hits, n, sat, ev = got
    exp = case.model(reads, p)
    assert len(n) == len(reads)
    for i, (res, s, e) in enumerate(exp):
        assert (int(n[i]), int(sat[i]), int(ev[i])) == (len(res), s, e), (p, i)
        w = min(len(res), max_results)
        assert [tuple(int(x) for x in hits[i, j]) for j in range(w)] == [tuple(r) for r in res[:w]], (p, i)
        assert not hits[i, w:].view(np.uint8).any(), (p, i)  # the rest of the row is zero
    return exp


@pytest.fixture(scope="module")
def cases(bf):
    return {(c, b): Case(bf, c, b, {"nt1": 6, "nt3": 17, "C5": 40}[c]) for c in CFGS for b in (2, 4)}


@pytest.mark.parametrize("cfg", list(CFGS))
def test_parameter_grid_ragged_host(cases, cfg):
    """the whole grid of the reference pin, uint16 ids, 64 ragged reads in host memory"""
    case = cases[cfg, 2]
    multi = sat = early = 0
    for p in param_sets(bool(case.seeds)):
        exp = check(case, case.reads, p, case.gpu(case.reads, p))
        multi += sum(len(r[0]) >= 2 for r in exp)
        sat += sum(r[1] > 0 for r in exp)
    assert multi and sat


@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_uint32_ids_fixed_layout_and_device(cases, cfg, device):
    """uint32 ids; a fixed read_len layout (reads padded with N to 120) and the ragged one; host and device inputs"""
    case = cases[cfg, 4]
    padded = [np.concatenate([s, np.full(120 - s.size, ord("N"), np.uint8)]) for s in case.reads]
    for p in param_sets(bool(case.seeds))[::5]:
        check(case, case.reads, p, case.gpu(case.reads, p, device=device))
        check(case, padded, p, case.gpu(padded, p, read_len=120, device=device))


def test_edge_reads_and_batch_split(cases, bf):
    """a read shorter than k, an all-N read, an empty read, a single-frame read; a small scratch budget that forces
    several batches changes nothing; an empty buffer"""
    case = cases["C5", 2]
    p = (1.0, 2, 1, 1, 0)
    g = case.reads
    reads = [g[0][:K - 1], np.full(60, ord("N"), np.uint8), np.zeros(0, np.uint8), g[1][:K]] + g[:20]
    exp = check(case, reads, p, case.gpu(reads, p))
    assert exp[0] == ([], 0, 0) and exp[1] == ([], 0, 0) and exp[2] == ([], 0, 0)
    assert exp[3][2] > 0  # the single frame was looked up
    whole = case.gpu(g, p)
    case.m.setScratchBudget(4096)
    try:
        split = case.gpu(g, p)
    finally:
        case.m.setScratchBudget(0)
    for a, b in zip(whole, split):
        assert (np.asarray(a) == np.asarray(b)).all()
    hits, n, sat, ev = case.m.classify(np.zeros(0, np.uint8), case.prob, case.minc, read_len=100)
    assert len(n) == 0
    case.m.setScratchBudget(64)
    try:
        with pytest.raises(bf._lib.BtlbfError) as ei:
            case.gpu(g, p)
        assert ei.value.code == bf._lib.ENOMEM
    finally:
        case.m.setScratchBudget(0)


def test_max_results_truncates_records_not_the_count(bf):
    case = Case(bf, "C5", 2, 12, share=3)  # three IDs share each common part
    p = (2.0, LARGE, 0, 1, 0)
    exp = case.model(case.reads, p)
    pick = [s for s, e in zip(case.reads, exp) if len(e[0]) >= 3]
    assert pick  # a read with three true results
    hits, n, sat, ev = case.gpu(pick, p, max_results=1)
    check(case, pick, p, (hits, n, sat, ev), max_results=1)
    assert int(n[0]) >= 3 and hits.shape[1] == 1


@pytest.fixture(scope="module")
def long_case(bf):
    """300 ids (301 table entries) and a contig of about 5000 bases over 50 of their genomes"""
    case = Case(bf, "C5", 2, 300, n_reads=0, bits=1 << 20, seed=9, length=100)
    rng = np.random.RandomState(3)
    contig = np.concatenate([ACGT[rng.randint(0, 4, 20)]] + genomes_of(np.random.RandomState(9), 300, 100)[:50])
    return case, contig


def test_long_sequence_takes_the_global_table(long_case):
    """about 5000 bases over about 300 ids: more distinct ids possible than an LDS table holds"""
    case, contig = long_case
    reads = [contig[:5000], contig[:80]]
    p = (1.0, LARGE, 1, 1, 0)
    check(case, reads, p, case.gpu(reads, p))
    assert case.m.classifyPaths() == (1, 1)


def test_global_table_in_a_later_batch(long_case):
    """three 80-base reads, then the 5000-base one, under a budget of 63000 bytes: the short reads cost 864 bytes each,
    the long one 62364 with its 512-slot table, so it is a batch of its own behind theirs (tests/cpp/test_mibf_plan.cpp
    asserts that plan for these lengths and this budget)"""
    case, contig = long_case
    reads = [contig[:80], contig[100:180], contig[200:280], contig[:5000]]
    assert [len(s) for s in reads] == [80, 80, 80, 5000] and case.n_ids == 301 and case.h == 4 and case.id_bytes == 2
    p = (1.0, LARGE, 1, 1, 0)
    whole = case.gpu(reads, p)
    check(case, reads, p, whole)
    assert case.m.classifyPaths() == (3, 1)
    case.m.setScratchBudget(63000)
    try:
        split = case.gpu(reads, p)
        paths = case.m.classifyPaths()
    finally:
        case.m.setScratchBudget(0)
    check(case, reads, p, split)
    for a, b in zip(whole, split):
        assert (np.asarray(a) == np.asarray(b)).all()
    assert paths == (3, 1)


def test_ids_beyond_the_tables_are_refused(cases, bf):
    """n_ids equal to the largest stored ID (the boundary: IDs must be < n_ids) and one below it: EINVAL, and no byte
    of the four outputs is written.  Then the argument errors."""
    case = cases["nt3", 2]
    top = int((case.data & 0x7FFF).max())
    seq = np.concatenate(case.reads[:4])
    starts = np.concatenate([[0], np.cumsum([len(s) for s in case.reads[:4]])]).astype(np.uint64)
    hits = np.full((4, 2, 4), 0xABABABAB, np.uint32)
    outs = [np.full(4, 7, np.uint32) for _ in range(3)]
    L = bf._lib
    import ctypes as C

    lay = L.Layout(C.c_void_p(starts.ctypes.data), 4, 0)
    par = L.MibfClassifyParams(1.0, 0, 0, 1, 0, 2)
    prob = np.zeros(top + 1, np.float64)
    minc = np.ones(top + 1, np.uint32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(par, n_ids):
        return L.load().btlbf_mibf_classify_seqs(case.m._h, ptr(seq), seq.size, C.byref(lay), C.byref(par), ptr(prob),
                                                 ptr(minc), n_ids, ptr(hits), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                                 L.HOST, None)

    for n_ids in (top, top - 1):
        assert call(par, n_ids) == L.EINVAL, n_ids
        assert (hits == 0xABABABAB).all() and all((o == 7).all() for o in outs), n_ids
    for bad in (dict(max_results=0), dict(n_ids=0), dict(n_ids=(1 << 15) + 1)):
        par2 = L.MibfClassifyParams(1.0, 0, 0, 1, 0, bad.get("max_results", 2))
        assert call(par2, bad.get("n_ids", top + 1)) == L.EINVAL, bad
        assert (hits == 0xABABABAB).all() and all((o == 7).all() for o in outs), bad
    assert call(par, top + 1) == 0  # the same call with tables that cover every stored ID goes through
    assert not (hits == 0xABABABAB).any() and not any((o == 7).all() for o in outs[1:])


@pytest.mark.parametrize("frames", [70000, 65536 + 65300])
def test_uint16_counters_wrap(bf, frames):
    """identical hit frames of one id, no early stop: the six counters wrap at 65536 as the reference's uint16_t do.
    After 70000 frames the id's counts (4464) are nowhere near the best counts seen (65535), so isValid drops the only
    candidate: no result, where counters that did not wrap would give one.  After 65536 + 65300 frames the counts are
    back within the standard error of the best, and the record shows the wrapped totalCount."""
    rng = np.random.RandomState(2)
    kmer = ACGT[rng.randint(0, 4, K)]
    f = bf.BloomFilter(1 << 12, 1, K)
    f.insertSeqs(kmer, read_len=K)
    ranks = mm.Ranks(f.download(), 1 << 12)
    m = bf.MIBloomFilter(f, 2)
    m.insertIDs(kmer, np.array([1]), read_len=K)
    seq = np.tile(np.concatenate([kmer, [ord("N")]]).astype(np.uint8), frames)  # every frame the same k-mer
    hits, n, sat, ev = m.classify(seq, [0.5, 0.25], [1, 1], extra_frame_limit=LARGE, starts=np.array([0, seq.size], np.uint64))
    rows = np.repeat(np.asarray(bf.hash_seqs(kmer, 1, K)[0])[:1].astype(np.uint64), frames, axis=0)
    res, s, e = cm.classify(m.data().astype(np.int64), ranks, rows, 2, False, [0.5, 0.25], [1, 1], extra_frame_limit=LARGE)
    assert e == 2 * frames and (int(sat[0]), int(ev[0])) == (s, e)
    assert int(n[0]) == len(res) == (0 if frames == 70000 else 1)
    if res:
        assert res[0][3] == frames - 65536 and tuple(int(x) for x in hits[0, 0]) == tuple(res[0])
