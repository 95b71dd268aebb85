"""The CPU restatement against the genuine reference build on fresh random inputs.
The reference's outputs on these seeded inputs are pinned by their SHA-256 in tests/golden/oracle_vs_ref.json, so the
tests run everywhere; where oracle/_ref/libbtlref.so exists they also compare against it live.  Re-record the file
from the reference with BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_oracle_vs_ref.py."""
import hashlib
import json
import os

import numpy as np
import pytest
from conftest import GOLDEN, load_golden

import large_k_cases as lk

GOLDEN_FILE = "oracle_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))


def sha_u64(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.asarray(a).astype(np.uint64).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def ref_or_none():
    from oracle import pyoracle

    if pyoracle.Ref.available():
        return pyoracle.Ref()
    if RECORD:
        pytest.fail("recording needs oracle/_ref/libbtlref.so")
    return None


@pytest.fixture(scope="module")
def pinned():
    """check(key, got, exp): the oracle's outputs `got` hash to the reference's recorded outputs; `exp` are the live
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


def rand_seq(rng, n, p_bad=0.02):
    s = rng.choice(list(b"ACGTacgt"), n).astype(np.uint8)
    bad = rng.rand(n) < p_bad
    s[bad] = rng.choice(list(b"NnRY-\x00\x01\x07\xff"), bad.sum())
    return s.tobytes()


@pytest.mark.parametrize("k,h", [(4, 5), (25, 3), (31, 4), (32, 2), (33, 1), (64, 4), (150, 2)])
def test_nthash_random(oracle, ref_or_none, pinned, k, h):
    ref = ref_or_none
    rng = np.random.RandomState(k * 100 + h)
    tot = 0
    got, exp = [], []
    for _ in range(60):
        s = rand_seq(rng, int(rng.randint(0, 600)), p_bad=rng.choice([0, 0.005, 0.05]))
        a = oracle.nthash_seq(s, h, k)
        got += [a[0], a[1]]
        if ref:
            b = ref.nthash_seq(s, h, k)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
            exp += [b[0], b[1]]
        tot += len(a[0])
    assert tot > 0
    pinned("nthash_k%d_h%d" % (k, h), got, exp if ref else None)


def test_kmer_path_random(oracle, ref_or_none, pinned):
    """raw k-mers (KmerBloomFilter's NTC64(kmerSeq, k) path): k 1..300, U, lowercase, bytes that are not bases"""
    ref = ref_or_none
    rng = np.random.RandomState(11)
    alpha = list(b"ACGT" * 5 + b"acgtUuNn\x01\x03-*")
    n_ok = n_skip = 0
    got, exp = [], []
    for it in range(6000):
        k = int(rng.randint(1, 300)) if it % 10 == 0 else int(rng.randint(1, 41))
        km = bytes(rng.choice(alpha, k).tolist())
        hv, ok = oracle.kmer_hashes(km, k, 4)
        if ok[0]:  # (the reference reads beyond its 2-/3-mer tables otherwise: nothing to compare)
            got.append(hv[0])
            if ref:
                b = ref.kmer_hashes(km, k, 4)
                assert (hv[0] == b).all(), (km, k)
                exp.append(b)
            n_ok += 1
        else:
            assert k % 4 in (2, 3)
            n_skip += 1
    assert n_ok > 4000 and n_skip > 0
    pinned("kmer_path", got, exp if ref else None)


@pytest.mark.parametrize("k,h2", [(7, 1), (7, 2), (31, 1), (31, 3)])
def test_sthash_random(oracle, ref_or_none, pinned, k, h2):
    ref = ref_or_none
    rng = np.random.RandomState(k + h2)
    seeds = []
    for _ in range(3):
        half = "".join(rng.choice(list("1101"), (k + 1) // 2))
        seeds.append((half + half[::-1][k % 2:])[:k])
    got, exp = [], []
    for _ in range(30):
        s = rand_seq(rng, int(rng.randint(0, 400)), p_bad=rng.choice([0, 0.01]))
        a = oracle.sthash_seq(s, seeds, h2, k)
        got += list(a)
        if ref:
            b = ref.sthash_seq(s, seeds, h2, k)
            assert all((x == y).all() for x, y in zip(a, b))
            exp += list(b)
    pinned("sthash_k%d_h2%d" % (k, h2), got, exp if ref else None)


# ---- large k: the sizes at which the GPU kernels change their code path (tests/test_gpu_large_k.py) ----------------
# Live against the genuine reference only (the `ref` fixture skips without oracle/_ref); tests/golden/large_k.json and
# test_oracle_golden.py carry the same pin to machines without it.  Every input holds an N, a lowercase run and one of
# the raw bytes 1 3 4 5 7 (large_k_cases.seq_recipe).
@pytest.mark.parametrize("case", [c for c in lk.golden_cases() if c["kind"] != "kmer"], ids=lambda c: c["name"])
def test_large_k_hash_streams(oracle, ref, case):
    a, b = lk.run_case(oracle, case), lk.run_case(ref, case)
    s = lk.build_input(case["input"])
    assert lk.N in s and any(x in s for x in lk.RAW_BYTES) and s != s.upper()
    # windows on either side of the N, none across it
    p = [q for q, byte in case["input"]["bytes"] if byte == lk.N][0]
    pos = a["pos"].astype(np.int64)
    assert (pos < p - case["k"] + 1).any() and (pos > p).any() and not ((pos > p - case["k"]) & (pos <= p)).any()
    for key in b:
        assert a[key].shape == b[key].shape and (a[key] == b[key]).all(), (case["name"], key)
    assert lk.digest_case(a) == load_golden(lk.GOLDEN_FILE)[case["name"]]["expected"]


@pytest.mark.parametrize("case", [c for c in lk.golden_cases() if c["kind"] == "kmer"], ids=lambda c: c["name"])
def test_large_k_kmer_path(oracle, ref, case):
    """raw k-mers at k = 1023 (k % 4 == 3), 1024 and 32768 (0), 4097 (1): lowercase, U, an N, a raw byte"""
    a, hv, ok = lk.kmer_case_outputs(oracle, case)
    b, _, _ = lk.kmer_case_outputs(oracle, case, ref)
    assert ok.sum() >= 6, ok
    assert (a["hashes"] == b["hashes"]).all(), case["name"]
    assert lk.digest_case(a) == load_golden(lk.GOLDEN_FILE)[case["name"]]["expected"]


@pytest.mark.parametrize("bits", [64, 1000, 1 << 16, 999992])
def test_bit_filter_ops(oracle, ref_or_none, pinned, bits):
    ref = ref_or_none
    rng = np.random.RandomState(bits % 9973)
    h = 4
    mine = np.zeros(bits // 8, np.uint8)
    hv = rng.randint(0, 2 ** 63, size=(500, h)).astype(np.uint64) * np.uint64(2) + rng.randint(0, 2, size=(500, h)).astype(np.uint64)
    got = [oracle.bf_insert_and_check(mine, bits, h, hv[:200])]
    oracle.bf_insert(mine, bits, h, hv[200:300])
    got += [mine, oracle.bf_contains(mine, bits, h, hv), [oracle.bf_popcount(mine, bits)]]
    exp = None
    if ref:
        f = ref.bf(bits, h, 31)
        exp = [f.insert_and_check(hv[:200])]
        f.insert(hv[200:300])
        exp += [f.bytes(), f.contains(hv), [f.pop()]]
        assert got[0].tolist() == exp[0].tolist()
        assert (mine == exp[1]).all()
        assert got[2].tolist() == exp[2].tolist()
        assert got[3] == exp[3]
    pinned("bit_filter_ops_%d" % bits, got, exp)


def test_counting_ops(oracle, ref_or_none, pinned):
    ref = ref_or_none
    rng = np.random.RandomState(5)
    h, thr = 3, 2
    f = ref.cbf(1001, h, 25, thr) if ref else None
    c = np.zeros(oracle.cbf_round_bytes(1001), np.uint8)
    assert c.size == 1008 and (f is None or f.size == 1008)
    got, exp = [], []
    for rnd in range(6):
        hv = rng.randint(0, 2 ** 62, size=(700, h)).astype(np.uint64)
        hv[::7, 1] = hv[::7, 0]  # duplicate positions inside one k-mer
        if rnd % 3 == 0:
            oracle.cbf_increment_min(c, h, hv)
            if f:
                f.insert(hv)
        elif rnd % 3 == 1:
            oracle.cbf_increment_all(c, h, hv)
            if f:
                f.increment_all(hv)
        else:
            got.append(oracle.cbf_insert_and_check(c, h, thr, hv))
            if f:
                exp.append(f.insert_and_check(hv))
                assert got[-1].tolist() == exp[-1].tolist()
        a = oracle.cbf_query(c, h, thr, hv)
        got += [c.copy(), a[0], a[1]]
        if f:
            b = f.query(hv)
            exp += [f.counters().copy(), b[0], b[1]]
            assert (c == exp[-3]).all()
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    got.append([oracle.cbf_popcount(c), oracle.cbf_filtered_popcount(c, thr)])
    if f:
        exp.append([f.popcount(), f.filtered_popcount()])
        assert got[-1] == exp[-1]
    pinned("counting_ops", got, exp if f else None)


def test_headers_and_files(oracle, ref_or_none, pinned, tmp_path):
    """the files the reference stores: header + body, the body built by the oracle from the same sequence"""
    ref = ref_or_none
    seq = b"ACGTTGCATGCATGCATGCAGTCAGTCGATGCATGCA"
    body = np.zeros(4096 // 8, np.uint8)
    oracle.bf_insert_seq(body, 4096, 7, 21, seq)
    got = [np.frombuffer(oracle.bf_header(4096, 7, 21, 0.0, 12, 34) + body.tobytes(), np.uint8),
           np.frombuffer(oracle.cbf_header(128, 128, 2, 9) + bytes(128), np.uint8)]
    exp = None
    if ref:
        f = ref.bf(4096, 7, 21)
        f.insert_seq(seq)
        f.set_entries(12, 34)
        p = str(tmp_path / "a.bf")
        f.store(p)
        raw = open(p, "rb").read()
        assert raw == oracle.bf_header(4096, 7, 21, 0.0, 12, 34) + f.bytes().tobytes()
        c = ref.cbf(123, 2, 9, 1)
        p2 = str(tmp_path / "c.bf")
        c.store(p2)
        raw2 = open(p2, "rb").read()
        assert raw2 == oracle.cbf_header(128, 128, 2, 9) + bytes(128)
        exp = [np.frombuffer(raw, np.uint8), np.frombuffer(raw2, np.uint8)]
    pinned("headers_and_files", got, exp)


def test_synth_reads(oracle, ref_or_none, pinned):
    ref = ref_or_none
    got, exp = [], []
    for seed, first, n, L in [(42, 0, 100, 150), (43, 10 ** 9, 10, 150), (1, 3, 7, 33), (9, 0, 5, 64)]:
        got.append(oracle.synth_reads(seed, first, n, L))
        if ref:
            exp.append(ref.synth_reads(seed, first, n, L))
            assert (got[-1] == exp[-1]).all()
    pinned("synth_reads", got, exp if ref else None)


def test_port_bench_matches_reference_bench(oracle, ref_or_none, pinned):
    ref = ref_or_none
    a = oracle.bench_bf(3000, 150, 31, 4, 1 << 24, 42, 43, threads=2)
    assert a["kmers"] == 3000 * 120
    exp = None
    if ref:
        b = ref.bench_bf(3000, 150, 31, 4, 1 << 24, 42, 43, threads=2, skip_pop=0)
        assert a["kmers"] == b["kmers"] == 3000 * 120
        assert a["hits"] == b["hits"] and a["popcount"] == b["popcount"]
        exp = [[b["kmers"], b["hits"], b["popcount"]]]
    pinned("port_bench", [[a["kmers"], a["hits"], a["popcount"]]], exp)
