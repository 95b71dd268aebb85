"""miBF stages 3-4 on the GPU (btlbf_mibf_*) against the numpy restatement of the reference in tests/mibf_model.py,
exactly: ID insertion, saturation (serial and parallel), query, statistics and the data file."""
import numpy as np
import pytest

import mibf_model as mm

pytestmark = pytest.mark.gpu

C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]
K = 31


@pytest.fixture(scope="module")
def bf():
    import torch

    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as m

    return m


def ragged(rng, n, lo=40, hi=200, n_rate=0.01):
    lens = rng.randint(lo, hi, n)
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, int(starts[-1]))].copy()
    seq[rng.rand(seq.size) < n_rate] = ord("N")
    return seq, starts


def stage1(bf, bits, h, seeds, seq, starts=None, read_len=0):
    f = bf.BloomFilter(bits, h, K)
    if seeds:
        f.setSpacedSeeds(seeds, 1)
    f.insertSeqs(seq, starts=starts, read_len=read_len)
    return f


def rows_of(bf, seq, h, seeds, starts=None, read_len=0):
    if seeds:
        hv, valid, _ = bf.sthash_seqs(seq, seeds, 1, K, starts=starts, read_len=read_len)
    else:
        hv, valid = bf.hash_seqs(seq, h, K, starts=starts, read_len=read_len)
    n = len(seq)
    return np.asarray(hv)[:n].astype(np.uint64), bf.bits_to_bool(valid, n)


def model_state(m):
    return np.zeros(m.getPop(), np.int64), np.zeros(m.getPop(), np.int64)


CFG = [(C5_SEEDS, 4), (None, 3)]


@pytest.mark.parametrize("seeds,h", CFG, ids=["C5", "nthash3"])
@pytest.mark.parametrize("id_bytes", [2, 4])
@pytest.mark.parametrize("bits", [1 << 18, 64 * 4099, 1234568])
def test_insert_ids_against_model(bf, seeds, h, id_bytes, bits):
    rng = np.random.RandomState(bits % 1000 + id_bytes + h)
    seq, starts = ragged(rng, 300)
    f = stage1(bf, bits, h, seeds, seq, starts=starts)
    body = f.download()
    m = bf.MIBloomFilter(f, id_bytes)
    f.close()  # the rank records hold the words
    ranks = mm.Ranks(body, bits)
    assert m.getPop() == ranks.pop and m.size() == bits and m.getHashNum() == h and m.getKmerSize() == K
    ids = rng.randint(1, 40, 300)  # repeated, non-monotone
    ids[::7] = 3
    m.insertIDs(seq, ids, starts=starts)
    rows, valid = rows_of(bf, seq, h, seeds, starts=starts)
    data, counts = model_state(m)
    mm.insert_ids(data, counts, ranks, rows, valid, mm.window_seqs(len(seq), starts), ids, id_bytes)
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()


def test_insert_ids_small_filter_and_split_calls(bf):
    """a filter so small that one sequence hits one rank with several hash values; the same input in one call and
    split over three calls (and over small batches of a tiny scratch budget) gives the same arrays"""
    rng = np.random.RandomState(5)
    seq, starts = ragged(rng, 60, 60, 120)
    bits = 512
    f = stage1(bf, bits, 4, C5_SEEDS, seq, starts=starts)
    ranks = mm.Ranks(f.download(), bits)
    ids = rng.randint(1, 1000, 60)
    rows, valid = rows_of(bf, seq, 4, C5_SEEDS, starts=starts)
    wseq = mm.window_seqs(len(seq), starts)
    rk = ranks.rank(rows[valid].ravel())
    s = np.repeat(wseq[valid], 4)
    pairs = np.unique(np.stack([s, rk, rows[valid].ravel().astype(np.int64)]), axis=1)
    _, cnt = np.unique(pairs[:2], axis=1, return_counts=True)
    assert cnt.max() >= 2  # one sequence, one rank, two distinct hash values
    a = bf.MIBloomFilter(f, 2)
    a.insertIDs(seq, ids, starts=starts)
    data, counts = model_state(a)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, 2)
    assert (a.data().astype(np.int64) == data).all() and (a.counts().astype(np.int64) == counts).all()
    b = bf.MIBloomFilter(f, 2)
    b.setScratchBudget(1 << 16)
    cut = [0, 20, 45, 60]
    for i in range(3):
        lo, hi = int(starts[cut[i]]), int(starts[cut[i + 1]])
        b.insertIDs(seq[lo:hi], ids[cut[i]:cut[i + 1]], starts=starts[cut[i]:cut[i + 1] + 1] - starts[cut[i]])
    assert (b.data() == a.data()).all() and (b.counts() == a.counts()).all()


def test_insert_ids_large(bf):
    """>= 2*10^7 hash values through the batched path (a 64 MiB scratch budget: several batches)"""
    import torch

    n, L = 45000, 150
    reads = bf.synth_reads_device(11, 0, n, L)
    bits = 1 << 27
    f = stage1(bf, bits, 4, C5_SEEDS, reads, read_len=L)
    torch.cuda.synchronize()
    ranks = mm.Ranks(f.download(), bits)
    m = bf.MIBloomFilter(f, 2)
    m.setScratchBudget(64 << 20)
    ids = (np.arange(n) // 1000 + 1).astype(np.uint32)
    m.insertIDs(reads, torch.from_numpy(ids.astype(np.int32)).cuda(), read_len=L)
    host = reads.cpu().numpy()
    rows, valid = rows_of(bf, host, 4, C5_SEEDS, read_len=L)
    assert valid.sum() * 4 >= 2 * 10 ** 7
    data, counts = model_state(m)
    mm.insert_ids(data, counts, ranks, rows, valid, mm.window_seqs(len(host), read_len=L), ids, 2)
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()


def dense_case(bf, id_bytes, seeds, h):
    rng = np.random.RandomState(17)
    seq, starts = ragged(rng, 400, 60, 160, 0.005)
    bits = 1 << 15  # dense: many k-mers per entry
    f = stage1(bf, bits, h, seeds, seq, starts=starts)
    ranks = mm.Ranks(f.download(), bits)
    ids = rng.randint(1, 60, 400)
    rows, valid = rows_of(bf, seq, h, seeds, starts=starts)
    wseq = mm.window_seqs(len(seq), starts)
    return seq, starts, f, ranks, ids, rows, valid, wseq


@pytest.mark.parametrize("serial", [True, False], ids=["serial", "parallel"])
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_saturation_against_model(bf, serial, id_bytes):
    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, id_bytes, C5_SEEDS, 4)
    m = bf.MIBloomFilter(f, id_bytes)
    m.insertIDs(seq, ids, starts=starts)
    data, counts = model_state(m)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert (m.data().astype(np.int64) == data).all()
    got = m.insertSaturation(seq, ids, starts=starts, serial=serial)
    fn = mm.saturate_serial if serial else mm.saturate_parallel
    exp = fn(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert [got["clean"], got["found"], got["mutated"], got["saturated"]] == exp
    assert exp[2] >= 0.01 * exp[0] and exp[3] >= 0.01 * exp[0] and exp[1] > 0  # all three outcomes
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()


def test_parallel_saturation_scratch_budget(bf):
    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, 2, C5_SEEDS, 4)
    from btl_bloomfilter_amd._lib import BtlbfError

    m = bf.MIBloomFilter(f, 2)
    m.insertIDs(seq, ids, starts=starts)
    before, cb = m.data(), m.counts()
    m.setScratchBudget(256)
    with pytest.raises(BtlbfError) as e:
        m.insertSaturation(seq, ids, starts=starts)
    assert e.value.code == 2
    assert (m.data() == before).all() and (m.counts() == cb).all()


@pytest.mark.parametrize("seeds,h", CFG, ids=["C5", "nthash3"])
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_query_against_model(bf, seeds, h, id_bytes):
    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, id_bytes, seeds, h)
    m = bf.MIBloomFilter(f, id_bytes)
    m.insertIDs(seq, ids, starts=starts)
    m.insertSaturation(seq, ids, starts=starts)
    rng = np.random.RandomState(3)
    foreign, fst = ragged(rng, 100, 40, 150, 0.02)
    q = np.concatenate([seq, foreign])
    qst = np.concatenate([starts, fst[1:] + starts[-1]]).astype(np.uint64)
    qrows, qvalid = rows_of(bf, q, h, seeds, starts=qst)
    data = m.data()
    seen = set()
    for mx in (0, 1, 2):
        vals, hit, vb, cnt = m.query(q, max_miss=mx, starts=qst, want_counts=True)
        ev, match = mm.query(data, ranks, qrows, qvalid, mx, bool(seeds))
        assert (bf.bits_to_bool(vb, len(q)) == qvalid).all()
        assert (bf.bits_to_bool(hit, len(q)) == match).all()
        assert (np.asarray(vals).astype(np.int64) == ev).all()
        assert cnt.tolist() == [int(qvalid.sum()), int(match.sum())]
        seen.add(int(match.sum()))
    if seeds:
        assert len(seen) == 3  # max_miss changes the answer
    else:
        assert len(seen) == 1  # ... and is ignored without seeds
    ident, sat = m.decode(vals)
    assert (ident == (ev & (m.mask - 1))).all() and (sat == (ev > m.mask)).all()


@pytest.mark.parametrize("id_bytes", [2, 4])
def test_stats_store_load(bf, id_bytes, tmp_path):
    from btl_bloomfilter_amd._lib import BtlbfError

    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, id_bytes, C5_SEEDS, 4)
    m = bf.MIBloomFilter(f, id_bytes)
    m.insertIDs(seq, ids, starts=starts)
    m.insertSaturation(seq, ids, starts=starts)
    d = m.data().copy()
    d[0] = m.mask  # == mask: not saturated (strict >)
    d[1] = m.mask + 1
    m.upload(d)
    assert (m.data() == d).all()
    nz, sat = mm.stats(d, id_bytes)
    assert m.getPopNonZero() == nz and m.getPopSaturated() == sat and m.getPop() == ranks.pop
    for n_ids in (61, 20000):
        hist, s2 = m.getIDCounts(n_ids)
        eh, es = mm.id_counts(d, n_ids, id_bytes)
        assert (hist == eh).all() and s2 == es == sat
    p = tmp_path / "x.mibf"
    m.store(p)
    assert p.read_bytes() == mm.file_bytes(d, id_bytes, 4, K, C5_SEEDS)
    m2 = bf.MIBloomFilter.load(p, f, id_bytes)
    assert (m2.data() == d).all() and m2.getPop() == m.getPop()
    q1 = m.query(seq, max_miss=1, starts=starts)[0]
    q2 = m2.query(seq, max_miss=1, starts=starts)[0]
    assert (np.asarray(q1) == np.asarray(q2)).all()
    # corrupted: the data length, the magic
    raw = p.read_bytes()
    for bad in (raw[:-1], b"MIBLOOMZ" + raw[8:]):
        p.write_bytes(bad)
        with pytest.raises(BtlbfError) as e:
            bf.MIBloomFilter.load(p, f, id_bytes)
        assert e.value.code == 4
    # a bit filter whose popcount is not the file's size
    p.write_bytes(raw)
    other = bf.BloomFilter(1 << 15, 4, K)
    other.setSpacedSeeds(C5_SEEDS, 1)
    with pytest.raises(BtlbfError) as e:
        bf.MIBloomFilter.load(p, other, id_bytes)
    assert e.value.code == 4


def test_spaced_seeds_need_h2_one(bf):
    from btl_bloomfilter_amd._lib import BtlbfError

    f = bf.BloomFilter(1 << 12, 8, K)
    f.setSpacedSeeds(C5_SEEDS, 2)
    with pytest.raises(BtlbfError) as e:
        bf.MIBloomFilter(f, 2)
    assert e.value.code == 1
