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


def stage1(bf, bits, h, seeds, seq, starts=None, read_len=0, k=K):
    f = bf.BloomFilter(bits, h, k)
    if seeds:
        f.setSpacedSeeds(seeds, 1)
    f.insertSeqs(seq, starts=starts, read_len=read_len)
    return f


def rows_of(bf, seq, h, seeds, starts=None, read_len=0, k=K):
    if seeds:
        hv, valid, _ = bf.sthash_seqs(seq, seeds, 1, k, starts=starts, read_len=read_len)
    else:
        hv, valid = bf.hash_seqs(seq, h, k, starts=starts, read_len=read_len)
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


def uniform_dense_case(bf):
    """300 reads of 100 bases in the fixed read_len layout over 2^15 bits (dense, as dense_case)"""
    rng = np.random.RandomState(29)
    L, n = 100, 300
    seq, _ = ragged(rng, n, L, L + 1, 0.005)
    ids = rng.randint(1, 50, n)
    f = stage1(bf, 1 << 15, 4, C5_SEEDS, seq, read_len=L)
    ranks = mm.Ranks(f.download(), 1 << 15)
    rows, valid = rows_of(bf, seq, 4, C5_SEEDS, read_len=L)
    return seq, L, f, ranks, ids, rows.reshape(len(seq), 4), valid, mm.window_seqs(len(seq), None, L)


@pytest.mark.parametrize("layout", ["ragged", "uniform"])
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_serial_saturation_in_many_batches(bf, id_bytes, layout):
    """the serial order under a scratch budget of 2^14 bytes: 496 bytes of sequence per batch (8 * 4 + 1 bytes of scratch
    per byte), so about a hundred batches of the ragged reads and 75 batches of four 100-base reads; arrays and counters
    as the model's single loop"""
    if layout == "ragged":
        seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, id_bytes, C5_SEEDS, 4)
        L = 0
    else:
        seq, L, f, ranks, ids, rows, valid, wseq = uniform_dense_case(bf)
        starts = None
    m = bf.MIBloomFilter(f, id_bytes)
    m.insertIDs(seq, ids, starts=starts, read_len=L)
    data, counts = model_state(m)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert (m.data().astype(np.int64) == data).all()
    m.setScratchBudget(1 << 14)
    got = m.insertSaturation(seq, ids, starts=starts, read_len=L, serial=True)
    exp = mm.saturate_serial(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert [got["clean"], got["found"], got["mutated"], got["saturated"]] == exp
    assert exp[2] >= 0.01 * exp[0] and exp[3] >= 0.01 * exp[0] and exp[1] > 0  # all three outcomes
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()


@pytest.mark.parametrize("budget", [256, "between"])
def test_serial_saturation_scratch_budget(bf, budget):
    """a read that does not fit the budget alone: ENOMEM before any batch has run, the arrays untouched.  256 bytes hold
    no read at all; the second budget holds the first reads and not a later, longer one"""
    seq, starts, f, ranks, ids, rows, valid, wseq = dense_case(bf, 2, C5_SEEDS, 4)
    from btl_bloomfilter_amd._lib import ENOMEM, BtlbfError

    lens = np.diff(starts.astype(np.int64))
    if budget == "between":
        fit = max(int(lens[:3].max()), int(np.median(lens)))  # bytes of sequence per batch
        assert lens.min() <= fit < lens.max() and (lens[:3] <= fit).all()
        budget = fit * (8 * 4 + 1)
    m = bf.MIBloomFilter(f, 2)
    m.insertIDs(seq, ids, starts=starts)
    before, cb = m.data(), m.counts()
    m.setScratchBudget(budget)
    with pytest.raises(BtlbfError) as e:
        m.insertSaturation(seq, ids, starts=starts, serial=True)
    assert e.value.code == ENOMEM
    assert (m.data() == before).all() and (m.counts() == cb).all()
    m.setScratchBudget(0)
    m.insertSaturation(seq, ids, starts=starts, serial=True)  # ... and the call was not a no-op by accident
    assert (m.data() != before).any()


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


# ---- edges: layouts, memory spaces, degenerate buffers, parameter limits, the counter's wrap ----------------------------


def three_ops(bf, m, ranks, data, counts, seq, ids, h, seeds, id_bytes, serial, max_misses, starts=None, read_len=0,
              device=False, k=K):
    """insertIDs, insertSaturation and query of one buffer on the miBF `m`, each against the model continued from
    (data, counts), which are updated in place; the buffer, its starts and its ids live on the device with device=True"""
    import torch

    seq = np.ascontiguousarray(seq, np.uint8)
    ids = np.asarray(ids, np.int64)
    rows, valid = rows_of(bf, seq, h, seeds, starts=starts, read_len=read_len, k=k)
    rows = rows.reshape(len(seq), h)
    wseq = mm.window_seqs(len(seq), starts, read_len)
    if device:
        dseq = torch.from_numpy(seq).cuda()
        dids = torch.from_numpy(ids.astype(np.int32)).cuda()
        dst = None if starts is None else torch.from_numpy(np.asarray(starts).astype(np.int64)).cuda()
    else:
        dseq, dids, dst = seq, ids, starts
    m.insertIDs(dseq, dids, starts=dst, read_len=read_len)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()
    got = m.insertSaturation(dseq, dids, starts=dst, read_len=read_len, serial=serial)
    exp = (mm.saturate_serial if serial else mm.saturate_parallel)(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    assert [got["clean"], got["found"], got["mutated"], got["saturated"]] == exp
    assert (m.counts().astype(np.int64) == counts).all()
    assert (m.data().astype(np.int64) == data).all()
    return exp, query_check(bf, m, ranks, data, seq, h, seeds, max_misses, starts=starts, read_len=read_len,
                            device=device, k=k)


def query_check(bf, m, ranks, data, seq, h, seeds, max_misses, starts=None, read_len=0, device=False, k=K):
    """query of one buffer for every max_miss against the model over `data` -> matching windows per max_miss"""
    import torch

    seq = np.ascontiguousarray(seq, np.uint8)
    rows, valid = rows_of(bf, seq, h, seeds, starts=starts, read_len=read_len, k=k)
    rows = rows.reshape(len(seq), h)
    dseq, dst = seq, starts
    if device:
        dseq = torch.from_numpy(seq).cuda()
        dst = None if starts is None else torch.from_numpy(np.asarray(starts).astype(np.int64)).cuda()
    n_match = []
    for mx in max_misses:
        vals, hit, vb, cnt = m.query(dseq, max_miss=mx, starts=dst, read_len=read_len, want_counts=True)
        if device:
            vals, hit, vb, cnt = (x.cpu().numpy() for x in (vals, hit, vb, cnt))
        ev, match = mm.query(data, ranks, rows, valid, mx, bool(seeds))
        assert (bf.bits_to_bool(vb, len(seq)) == valid).all()
        assert (bf.bits_to_bool(hit, len(seq)) == match).all()
        assert (np.asarray(vals).view(m.dtype).reshape(len(seq), h).astype(np.int64) == ev).all()
        assert [int(x) for x in cnt] == [int(valid.sum()), int(match.sum())]
        n_match.append(int(match.sum()))
    return n_match


@pytest.mark.parametrize("serial", [True, False], ids=["serial", "parallel"])
@pytest.mark.parametrize("layout,device", [("uniform", False), ("uniform", True), ("ragged", True)],
                         ids=["uniform-host", "uniform-device", "ragged-device"])
def test_layouts_and_device_inputs(bf, layout, device, serial):
    """the uniform layout and device-resident buffers through insertSaturation and query too (dense: all three outcomes);
    the query also over foreign sequences in the same layout, where max_miss changes the answer"""
    rng = np.random.RandomState(29)
    if layout == "uniform":
        L, n = 100, 300
        seq, starts = ragged(rng, n, L, L + 1, 0.005)
    else:
        L, n = 0, 300
        seq, starts = ragged(rng, n, 40, 160, 0.005)
    ids = rng.randint(1, 50, n)
    foreign, fst = ragged(rng, 60, L or 40, L + 1 if L else 160, 0.02)
    q, qst = np.concatenate([seq, foreign]), np.concatenate([starts, fst[1:] + starts[-1]]).astype(np.uint64)
    if L:
        starts = qst = None
    bits = 1 << 15
    f = stage1(bf, bits, 4, C5_SEEDS, seq, starts=starts, read_len=L)
    ranks = mm.Ranks(f.download(), bits)
    m = bf.MIBloomFilter(f, 2)
    data, counts = model_state(m)
    exp, n_match = three_ops(bf, m, ranks, data, counts, seq, ids, 4, C5_SEEDS, 2, serial, (0, 2), starts=starts,
                             read_len=L, device=device)
    assert min(exp[1:]) >= 0.01 * exp[0]
    assert n_match == [exp[0]] * 2  # every bit of an inserted window is set: max_miss cannot matter here
    n_match = query_check(bf, m, ranks, data, q, 4, C5_SEEDS, (0, 1, 2), starts=qst, read_len=L, device=device)
    assert len(set(n_match)) == 3


def _degenerate(name, rng):
    """-> (buffer, starts or None, read_len)"""
    real = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, n)].copy()  # noqa: E731
    if name == "empty":
        return np.zeros(0, np.uint8), np.zeros(2, np.uint64), 0  # no byte at all: one sequence of length zero
    if name == "shorter_than_k":
        lens = rng.randint(0, K, 50)
        return real(int(lens.sum())), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), 0
    if name == "only_n":
        return np.full(500, ord("N"), np.uint8), np.array([0, 100, 131, 500], np.uint64), 0
    if name == "only_n_uniform":
        return np.full(500, ord("N"), np.uint8), None, 50
    if name == "zero_length_between":
        return real(200), np.array([0, 90, 90, 200], np.uint64), 0
    assert name == "read_len_k"
    return real(40 * K), None, K


@pytest.mark.parametrize("serial", [True, False], ids=["serial", "parallel"])
@pytest.mark.parametrize("name", ["empty", "shorter_than_k", "only_n", "only_n_uniform", "zero_length_between",
                                  "read_len_k"])
def test_degenerate_buffers(bf, name, serial):
    """buffers with no clean window leave data and counts as they were and count nothing; a zero-length sequence keeps
    its id out of its neighbours' windows; read_len = k is one window per sequence"""
    rng = np.random.RandomState(31)
    base, bst = ragged(rng, 80, 60, 120, 0.005)
    buf, starts, L = _degenerate(name, rng)
    bits = 1 << 12
    f = stage1(bf, bits, 4, C5_SEEDS, base, starts=bst)
    if len(buf):
        f.insertSeqs(buf, starts=starts, read_len=L)
    ranks = mm.Ranks(f.download(), bits)
    m = bf.MIBloomFilter(f, 2)
    data, counts = model_state(m)
    bids = rng.randint(1, 30, 80)
    three_ops(bf, m, ranks, data, counts, base, bids, 4, C5_SEEDS, 2, serial, (1,), starts=bst)
    before = data.copy(), counts.copy()
    n_seqs = len(starts) - 1 if starts is not None else len(buf) // L
    ids = rng.randint(30, 60, n_seqs)
    exp, n_match = three_ops(bf, m, ranks, data, counts, buf, ids, 4, C5_SEEDS, 2, serial, (0, 1), starts=starts,
                             read_len=L)
    if name in ("zero_length_between", "read_len_k"):
        assert exp[0] == (200 - 2 * (K - 1) if name == "zero_length_between" else 40)
        assert (counts != before[1]).any()
    else:
        assert exp == [0, 0, 0, 0] and n_match == [0, 0]
        assert (data == before[0]).all() and (counts == before[1]).all()  # and three_ops compared the device's with them


@pytest.mark.parametrize("seeds,h,k,max_misses", [(None, 1, K, (0, 3)), (C5_SEEDS, 4, K, (3, 4, 5, 1 << 30)),
                                                  (None, 3, 32, (0,)), (None, 3, 33, (0,))],
                         ids=["nthash1", "C5-max_miss>=h", "nthash-k32", "nthash-k33"])
@pytest.mark.parametrize("id_bytes", [2, 4])
def test_parameter_edges(bf, seeds, h, k, max_misses, id_bytes):
    """one hash without seeds; max_miss at and beyond h with seeds (every clean window matches); k on both sides of the
    32 / 33 boundary of ntHash's split rotation"""
    rng = np.random.RandomState(37 + k + h)
    seq, starts = ragged(rng, 200, 40, 160, 0.01)
    bits = (1 << 13) * h
    f = stage1(bf, bits, h, seeds, seq, starts=starts, k=k)
    ranks = mm.Ranks(f.download(), bits)
    m = bf.MIBloomFilter(f, id_bytes)
    assert m.getHashNum() == h and m.getKmerSize() == k
    data, counts = model_state(m)
    ids = rng.randint(1, 40, 200)
    three_ops(bf, m, ranks, data, counts, seq, ids, h, seeds, id_bytes, True, (0,), starts=starts, k=k)
    foreign, fst = ragged(rng, 60, 40, 160, 0.02)
    rows, valid = rows_of(bf, foreign, h, seeds, starts=fst, k=k)
    for mx in max_misses:
        vals, hit, vb, cnt = m.query(foreign, max_miss=mx, starts=fst, want_counts=True)
        ev, match = mm.query(data, ranks, rows, valid, mx, bool(seeds))
        assert (bf.bits_to_bool(vb, len(foreign)) == valid).all()
        assert (bf.bits_to_bool(hit, len(foreign)) == match).all()
        assert (np.asarray(vals).astype(np.int64) == ev).all()
        assert cnt.tolist() == [int(valid.sum()), int(match.sum())]
        if seeds and mx >= h:
            assert (match == valid).all() and 0 < (ev != 0).sum() < ev.size
        else:
            assert 0 < match.sum() < valid.sum()


def test_insert_ids_counter_wrap_u16(bf):
    """uint16_t counts that wrap: a 64-bit stage-1 filter (64 ranks) under 9200 reads of 150 bases, whose 4.4 * 10^6
    distinct hash values give every rank more than 65 535 arrivals (at least 68 350 each: counted on the CPU from the
    same generator).  A count that wraps to 0 replaces nothing, and the next arrival counts as the first
    (include/btlbf.h).  One call, and three calls under a scratch budget of a few hundred reads per batch."""
    import torch

    n, L, bits = 9200, 150, 64
    reads = bf.synth_reads_device(23, 0, n, L)
    f = stage1(bf, bits, 4, C5_SEEDS, reads[: 100 * L], read_len=L)
    torch.cuda.synchronize()
    ranks = mm.Ranks(f.download(), bits)
    assert ranks.pop == 64
    ids = (np.arange(n) // 100 + 1).astype(np.uint32)
    dids = torch.from_numpy(ids.astype(np.int32)).cuda()
    host = reads.cpu().numpy()
    rows, valid = rows_of(bf, host, 4, C5_SEEDS, read_len=L)
    arrivals = np.bincount(ranks.rank(np.unique(rows[valid].ravel())), minlength=64)  # distinct values alone
    assert arrivals.min() > 65535  # from the model's inputs alone: every one of the 64 counts wraps
    data, counts = np.zeros(64, np.int64), np.zeros(64, np.int64)
    mm.insert_ids(data, counts, ranks, rows, valid, mm.window_seqs(len(host), read_len=L), ids, 2)
    assert (counts < arrivals).all()
    a = bf.MIBloomFilter(f, 2)
    a.insertIDs(reads, dids, read_len=L)
    assert (a.counts().astype(np.int64) == counts).all()
    assert (a.data().astype(np.int64) == data).all()
    b = bf.MIBloomFilter(f, 2)
    b.setScratchBudget(8 << 20)
    for lo, hi in ((0, 3000), (3000, 3001), (3001, n)):
        b.insertIDs(reads[lo * L:hi * L], dids[lo:hi], read_len=L)
    assert (b.counts().astype(np.int64) == counts).all()
    assert (b.data().astype(np.int64) == data).all()
