"""The numpy miBF model (tests/mibf_model.py, the checker of tests/test_gpu_mibf.py) against the genuine reference:
MIBFConstructSupport<T, H> and MIBloomFilter<T> compiled behind oracle/ref_mibf_driver.cpp over the stand-ins of
oracle/standin/ for sdsl-lite and google sparsehash.

The reference's outputs on these seeded inputs are pinned by their SHA-256 in tests/golden/mibf_vs_ref.json, so the tests
run everywhere; where oracle/_ref/libbtlref.so has the miBF entry points they also compare against it live.  The pins
were recorded from the reference build, never from the model, with
    BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_mibf_vs_ref.py

What rests on the reference and what on this library's choice.  insertMIBF walks one sequence's distinct hash values in
the order of google::dense_hash_set, which depends on sparsehash's table; the stand-in walks them in ascending order,
the order include/btlbf.h defines.  The order changes the result only when one sequence puts two distinct values on one
rank.  Cases whose keys start with ``ref_`` use inputs for which this test computes that NO (sequence, rank) pair has
two distinct values (asserted): their pins hold for any walk order, i.e. for the genuine reference.  Cases whose keys
start with ``standin_order_`` have such pairs (asserted too) and check the ascending order this library defines, with
everything else (reservoir rule, setData, setSatIfMissing, rank, atRank, getPop, the file) still the reference's text.
The rank is the stand-in's: the ones of [0, i), as sdsl documents rank_support_il<1>.

The T counter's wrap cannot be pinned here: in the reference a wrapped count is a division by zero
(MIBFConstructSupport.hpp:125); the rule for it is this library's (include/btlbf.h), checked in test_mibf_cpu.py."""
import hashlib
import json
import math
import os

import numpy as np
import pytest
from conftest import GOLDEN, load_golden

import mibf_model as mm

GOLDEN_FILE = "mibf_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))
C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]
K = 31
CFGS = {"nt1": (None, 1), "nt3": (None, 3), "C5": (C5_SEEDS, 4)}


def sha_u64(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a).astype(np.uint64).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle import pyoracle

    if pyoracle.Ref.available():
        r = pyoracle.Ref()
        if r.has_mibf():
            return r
    if RECORD:
        pytest.fail("recording needs oracle/_ref/libbtlref.so with the miBF entry points")
    return None


@pytest.fixture(scope="module")
def pinned():
    """check(key, got, exp): the model's outputs `got` hash to the reference's recorded outputs; `exp` are the live
    reference's outputs where it is built (recorded in place of the file's value under BTLBF_RECORD_REF_GOLDEN)"""
    table = {} if RECORD else load_golden(GOLDEN_FILE)

    def check(key, got, exp=None):
        if RECORD:
            table[key] = sha_u64(exp)
        if exp is not None:
            assert sha_u64(got) == sha_u64(exp), key
        assert sha_u64(got) == table[key], key

    yield check
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump(dict(sorted(table.items())), f, indent=1)
            f.write("\n")


def with_n(rng, s, rate=0.01):
    s = s.copy()
    s[rng.rand(s.size) < rate] = ord("N")
    return s.tobytes()


def rand_bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, n)].copy()


def lengths(rng, n):
    """40-200 bases, every seventh sequence shorter than k"""
    lens = rng.randint(40, 201, n)
    lens[3::7] = rng.randint(0, K, len(lens[3::7]))
    return lens


def make_inputs(regime, h, seed):
    """-> (sequences, ids, expected_entries, occupancy, query sequences).  IDs repeat and are not monotone."""
    rng = np.random.RandomState(seed)
    if regime == "ref_low":
        # independent random sequences in a filter sized for far more entries than it gets: occupancy parameter 0.1,
        # nearly every entry has one owner, and (the point of the size) no sequence meets itself on a rank
        seqs = [with_n(rng, rand_bases(rng, n)) for n in lengths(rng, 25)]
        ids = rng.randint(1, 12, len(seqs))
        entries, occ = 6000 * h * h, 0.1
    elif regime == "ref_dense":
        # reads of one short genome at about 6-fold coverage with six ids: every entry has several owners with different
        # ids (the regime of test_gpu_mibf.dense_case: found, mutated and saturated all occur), from SHARED values rather
        # than from collisions, so that still no sequence meets itself on a rank.  expected_entries (300) is far below
        # the k-mer count of the reads (about 3500); the occupancy parameter is what makes the filter large.
        genome = rand_bases(rng, 800)
        seqs = []
        for n in lengths(rng, 60):
            o = rng.randint(0, genome.size - n + 1)
            seqs.append(with_n(rng, genome[o:o + n]))
        ids = rng.randint(1, 7, len(seqs))
        entries = 300
        occ = 1.0 - math.exp(-entries * h / (5e5 * h * h))
    else:
        # standin_order_dense: test_gpu_mibf.dense_case's regime by collisions: independent random sequences, expected_entries
        # far below their k-mer count (about 10000)
        assert regime == "standin_order_dense"
        seqs = [with_n(rng, rand_bases(rng, n), 0.005) for n in rng.randint(60, 160, 150)]
        ids = rng.randint(1, 60, len(seqs))
        entries, occ = 600, 0.25
    ids[::7] = 3
    # queries: inserted sequences, inserted sequences with substitutions (partial hits under spaced seeds), foreign ones
    q = [seqs[i] for i in range(0, 12, 2)]
    for i in range(1, 12, 2):
        s = np.frombuffer(seqs[i], np.uint8).copy()
        if s.size:
            at = rng.randint(0, s.size, 2)
            s[at] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), s[at]) + 1) % 4]
        q.append(s.tobytes())
    q += [with_n(rng, rand_bases(rng, n), 0.02) for n in (150, 31, 30, 90, 0)]
    return seqs, ids, entries, occ, q


# seeds of the ref_ inputs: chosen, by computing it, so that no (sequence, rank) pair has two distinct values
SEEDS = {("ref_low", "nt1"): 2, ("ref_low", "nt3"): 1, ("ref_low", "C5"): 1,
         ("ref_dense", "nt1"): 1, ("ref_dense", "nt3"): 1, ("ref_dense", "C5"): 1,
         ("standin_order_dense", "nt1"): 1, ("standin_order_dense", "nt3"): 1, ("standin_order_dense", "C5"): 1}


def rows_of(oracle, seqs, seeds, h):
    """hash rows of the emitted windows of every sequence, in order, and each row's sequence index: the rows come from
    oracle.nthash_seq / oracle.sthash_seq, pinned to the reference by test_oracle_vs_ref.py"""
    rows, wseq = [np.zeros((0, h), np.uint64)], [np.zeros(0, np.int64)]
    for i, s in enumerate(seqs):
        hv = oracle.sthash_seq(s, seeds, 1, K)[1] if seeds else oracle.nthash_seq(s, h, K)[1]
        rows.append(hv)
        wseq.append(np.full(len(hv), i, np.int64))
    return np.concatenate(rows), np.concatenate(wseq)


def shared_rank_pairs(ranks, rows, wseq):
    """number of (sequence, rank) pairs that receive two or more distinct hash values"""
    h = rows.shape[1]
    t = np.unique(np.stack([np.repeat(wseq, h), ranks.rank(rows.ravel()), rows.ravel().astype(np.int64)]), axis=1)
    _, cnt = np.unique(t[:2], axis=1, return_counts=True)
    return int((cnt >= 2).sum())


def optimal_size(entries, h, occupancy):
    """used ONLY where the reference is not built, and then only after its result matched the pinned digest of the
    size the reference's constructor reported (MIBloomFilter.hpp:84-88)"""
    v = int(-float(entries) * float(h) / math.log(1.0 - occupancy))
    return v + (64 - v % 64)


@pytest.mark.parametrize("id_bytes", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("cfg", list(CFGS))
@pytest.mark.parametrize("regime", ["ref_low", "ref_dense", "standin_order_dense"])
def test_model_against_reference(oracle, ref_or_none, pinned, tmp_path, regime, cfg, id_bytes):
    ref = ref_or_none
    seeds, h = CFGS[cfg]
    key = "%s_%s_u%d_" % (regime, cfg, 8 * id_bytes)
    seqs, ids, entries, occ, queries = make_inputs(regime, h, SEEDS[regime, cfg])
    assert any(len(s) < K for s in seqs) or regime == "standin_order_dense"
    if regime != "ref_low" and id_bytes == 2:
        # an id equal to s_mask: an entry that holds it is == mask, NOT > mask, so setData drops no bit onto its successor
        # and getPopSaturated does not count it.  uint16_t only: getIDCounts indexes its table by the entry's value, and a
        # table of 2^31 + 1 entries is not something to allocate
        ids[9::20] = mm.masks(id_bytes)[0]
        # id 0, uint16_t only for the same reason (a saturated 0 is == mask): entries that read as empty but have a count,
        # which is where setSatIfMissing's h leading zeros of seenSet / replacementIDs decide -- they make such an entry a
        # candidate, and with h = 1 they are the only candidates there are
        ids[4::10] = 0
    rows, wseq = rows_of(oracle, seqs, seeds, h)
    valid = np.ones(len(rows), bool)
    assert len(rows) > 10 * entries or regime == "ref_low"  # expected_entries far below the k-mer count

    # stage 1: the constructor's size, insertBV, getEmptyMIBF
    r = None
    if ref:
        r = ref.mibf(id_bytes, entries, K, h, occ, seeds)
        for s in seqs:
            r.insert_bv(s)
        r.get_empty()
        size = r.filter_size()
        assert r.stats()[0] == size
    else:
        size = optimal_size(entries, h, occ)
    pinned(key + "size", [size], [size] if r else None)
    bits = np.zeros((size + 7) // 8 * 8, np.uint8)  # insertBV: bit hash % size of every value
    bits[(rows.ravel() % np.uint64(size)).astype(np.int64)] = 1
    mine = np.packbits(bits, bitorder="little")[: (size + 7) // 8]
    body = r.body() if r else mine
    pinned(key + "bv", [mine], [body] if r else None)
    ranks = mm.Ranks(body, size)  # live: over the reference's own bit-vector bytes
    pinned(key + "pop", [ranks.pop], [r.stats()[1]] if r else None)

    pairs = shared_rank_pairs(ranks, rows, wseq)
    if regime.startswith("ref_"):
        assert pairs == 0  # the walk order of a sequence's values cannot matter: these pins are the reference's
    else:
        assert pairs >= 10  # ... here it does: the ascending order of the stand-in, which include/btlbf.h defines

    # stage 3: insertMIBF per (sequence, id)
    data, counts = np.zeros(ranks.pop, np.int64), np.zeros(ranks.pop, np.int64)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    exp = None
    if r:
        for s, i in zip(seqs, ids):
            r.insert_mibf(s, i)
        exp = [r.data(), r.stats()[2:]]
        assert (data == exp[0]).all(), key
    pinned(key + "ids", [data, mm.stats(data, id_bytes)], exp)
    owners = np.bincount(ranks.rank(np.unique(rows.ravel())), minlength=ranks.pop)
    if regime == "ref_low":
        assert (owners == 1).mean() > 0.95  # nearly all entries have a single owner
    else:
        assert (counts > 1).mean() > 0.5

    # stage 4: insertSaturation per (sequence, id), single-threaded
    out = mm.saturate_serial(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    n_ids = int(ids.max()) + 1
    hist, sat = mm.id_counts(data, n_ids, id_bytes)
    exp = None
    if r:
        for s, i in zip(seqs, ids):
            r.insert_saturation(s, i)
        eh, es = r.id_counts(n_ids)
        exp = [r.data(), r.stats()[2:], eh, [es]]
        assert (data == exp[0]).all(), key
    pinned(key + "saturation", [data, mm.stats(data, id_bytes), hist, [sat]], exp)
    if regime != "ref_low":
        # the inputs must reach every outcome (else they are wrong, not the model); the counts are the model's, whose
        # arrays have just been matched with the reference's own
        clean, found, mutated, saturated = out
        assert clean == len(rows)
        assert found >= 0.01 * clean and saturated >= 0.01 * clean, out
        if h == 1 and id_bytes == 4:
            # no mutation is possible with one hash unless an entry reads as 0: replacementIDs then holds only its zeros,
            # and without id 0 no entry is 0 once every sequence has been through insertMIBF
            assert mutated == 0
        else:
            assert mutated >= 0.01 * clean, out

    # atRank, both overloads, over inserted, altered and foreign sequences
    qrows, qseq = rows_of(oracle, queries, seeds, h)
    qvalid = np.ones(len(qrows), bool)
    n_match = set()
    for mx in (0, 1, 2, h):
        vals, match = mm.query(data, ranks, qrows, qvalid, mx, True)
        vals0, match0 = mm.query(data, ranks, qrows, qvalid, mx, False)
        exp = None
        if r:
            a = [r.at_rank(s, mx) for s in queries]
            ok0 = np.concatenate([x[1] for x in a]).astype(bool)
            ev0 = np.concatenate([x[2] for x in a])
            flag = np.concatenate([x[3] for x in a]) <= mx
            ev = np.where(flag[:, None], np.concatenate([x[5] for x in a]), 0)
            assert sum(len(x[0]) for x in a) == len(qrows)
            exp = [flag, ev, ok0, ev0]
        pinned(key + "at_rank_%d" % mx, [match, vals, match0, vals0], exp)
        n_match.add(int(match.sum()))
        assert 0 < match0.sum() < len(qrows)
    assert len(n_match) > 1 or h == 1  # max_miss changes the answer

    # the main file of store()
    got = mm.file_bytes(data, id_bytes, h, K, seeds or ())
    exp = None
    if r:
        p = tmp_path / "x.mibf"
        r.store(p)
        exp = [np.frombuffer(p.read_bytes(), np.uint8)]
        assert p.read_bytes() == got
        r.close()
    pinned(key + "file", [np.frombuffer(got, np.uint8)], exp)
