"""The classification model (tests/mibf_classify_model.py, the checker of tests/test_gpu_mibf_classify.py) against the
genuine reference: MIBFQuerySupport<T>::query compiled behind tests/cpp/ref_mibf_classify_driver.cpp over the stand-ins
of oracle/standin/ (sdsl, sparsehash) and tests/cpp/standin/ (boost's binomial, which only has to compile).

The reference's outputs on these seeded inputs are pinned in tests/golden/mibf_classify_vs_ref.json (a digest per
parameter set, and the figures the conditions below are asserted on), so the tests run everywhere; where the reference
tree is present the driver is built and compared live as well.  The pins were recorded from the reference build, never
from the model, with
    BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_mibf_classify_vs_ref.py

The miBF under the queries is built by the model's own insert_ids / saturate_serial (pinned by test_mibf_vs_ref.py); live,
its data array is compared with the driver's.

Conditions on the reference's output, per parameter set, so that no case passes vacuously: at least half of the reads have
a result, one has two, one has satCount > 0, and -- in the sets whose extra_frame_limit can be reached (0 and 2; with the
large limit the reference never stops early, by construction) -- one read stops early, its evalCount below that of the
same query without the stop.  Over the whole file at least one read is emptied by best_hit_agree.

extra_count is a power of two in every set: a reference built with contraction may fuse a - sqrt(a) * extra_count, and
with such a factor the fused and the unfused result are the same double."""
import hashlib
import itertools
import json
import math
import os
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, load_golden

import mibf_classify_model as cm
import mibf_model as mm

GOLDEN_FILE = "mibf_classify_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))
REF_DIR = os.environ.get("BTLBF_REFERENCE_DIR", "/root/reference")
C5_SEEDS = ["1110111011101110111011101110111", "1101101101101101011011011011011",
            "1111001111001111111001111001111", "1011101011101011101011101011101"]
K = 31
CFGS = {"nt1": (None, 1), "nt3": (None, 3), "C5": (C5_SEEDS, 4)}
LARGE = 1 << 30


def param_sets(spaced):
    """(extra_count, extra_frame_limit, max_miss, min_count, best_hit_agree): every extra_count x limit, min_count
    alternating, each with best_hit_agree off and on (the pair shows what the flag empties); seeds: max_miss 0 and 1"""
    out = []
    for mx in ((0, 1) if spaced else (0,)):
        for i, (ec, lim) in enumerate(itertools.product((0.5, 1.0, 2.0), (0, 2, LARGE))):
            for agree in (0, 1):
                out.append((ec, lim, mx, 1 if i % 2 == 0 else 3, agree))
    return out


# seeds of the inputs: the first of 0, 1, 2, ... with which the REFERENCE's output meets the conditions of the docstring
SEEDS = {("nt1", 2): 15, ("nt1", 4): 15, ("nt3", 2): 0, ("nt3", 4): 0, ("C5", 2): 2, ("C5", 4): 3}


def make_case(cfg, id_bytes):
    """IDs that share k-mers: every ID has a part of its own and a part it shares with one neighbour, so that entries have
    several owners (saturation) and reads hit several IDs.  -> (insert sequences, ids, entries, occupancy, reads,
    per_frame_prob, min_count_per_id)"""
    seeds, h = CFGS[cfg]
    rng = np.random.RandomState(SEEDS[cfg, id_bytes])
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n_ids = {"nt1": 6, "nt3": 17, "C5": 40}[cfg]
    shared = [acgt[rng.randint(0, 4, 110)] for _ in range((n_ids + 1) // 2)]
    genomes = [np.concatenate([acgt[rng.randint(0, 4, 150)], shared[i // 2], acgt[rng.randint(0, 4, 90)]]) for i in range(n_ids)]
    ids = np.arange(1, n_ids + 1)
    reads = []
    for r in range(24):
        i = rng.randint(0, n_ids)
        g = genomes[i]
        n = rng.randint(40, 121)
        if r % 3 == 0:  # across the junction of the ID's own part and the part it shares with its neighbour
            o = rng.randint(max(0, 190 - n), min(150, g.size - n) + 1)
        elif r % 3 == 1:  # a chimera of two IDs
            g = np.concatenate([g[:n // 2], genomes[(i + 3) % n_ids][200:200 + n - n // 2]])
            o = 0
        else:
            o = rng.randint(0, g.size - n + 1)
        s = g[o:o + n].copy()
        if r % 4 == 0:
            s[rng.randint(0, n)] = ord("N")
        reads.append(s.tobytes())
    prob = [0.001 * (i + 1) for i in range(n_ids + 1)]
    minc = [1 + i % 3 for i in range(n_ids + 1)]
    return [g.tobytes() for g in genomes], ids, 400 * n_ids, 0.3, reads, prob, minc


def optimal_size(entries, h, occupancy):
    """MIBloomFilter.hpp:84-88; used only after it matched the pinned size the reference's constructor reported"""
    v = int(-float(entries) * float(h) / math.log(1.0 - occupancy))
    return v + (64 - v % 64)


def rows_of(oracle, s, seeds, h):
    return oracle.sthash_seq(s, seeds, 1, K)[1] if seeds else oracle.nthash_seq(s, h, K)[1]


def build_model_mibf(oracle, cfg, id_bytes, size):
    seeds, h = CFGS[cfg]
    seqs, ids, _, _, _, _, _ = make_case(cfg, id_bytes)
    rows = np.concatenate([rows_of(oracle, s, seeds, h) for s in seqs])
    wseq = np.concatenate([np.full(len(rows_of(oracle, s, seeds, h)), i, np.int64) for i, s in enumerate(seqs)])
    bits = np.zeros((size + 7) // 8 * 8, np.uint8)
    bits[(rows.ravel() % np.uint64(size)).astype(np.int64)] = 1
    ranks = mm.Ranks(np.packbits(bits, bitorder="little")[: (size + 7) // 8], size)
    data, counts = np.zeros(ranks.pop, np.int64), np.zeros(ranks.pop, np.int64)
    valid = np.ones(len(rows), bool)
    mm.insert_ids(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    mm.saturate_serial(data, counts, ranks, rows, valid, wseq, ids, id_bytes)
    return ranks, data


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the reference driver, built where the reference tree lies; None elsewhere"""
    if not os.path.exists(os.path.join(REF_DIR, "MIBFQuerySupport.hpp")):
        if RECORD:
            pytest.fail("recording needs the reference tree")
        return None
    exe = str(tmp_path_factory.mktemp("refcls") / "ref_mibf_classify_driver")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-w", "-fno-access-control", "-I" + REF_DIR,
                        "-I" + os.path.join(ROOT, "oracle", "standin"), "-I" + os.path.join(ROOT, "tests", "cpp", "standin"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_mibf_classify_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, tmp_path, cfg, id_bytes):
    seeds, h = CFGS[cfg]
    seqs, ids, entries, occ, reads, prob, minc = make_case(cfg, id_bytes)
    ps = param_sets(bool(seeds))
    lines = ["%d %d %d %d %s %d %r" % (id_bytes, K, h, len(seeds or ()), " ".join(seeds or ()), entries, occ), str(len(seqs))]
    lines += ["%d %s" % (i, s.decode() or "-") for i, s in zip(ids, seqs)]
    lines += [str(len(prob))] + ["%r %d" % (p, m) for p, m in zip(prob, minc)]
    lines += [str(len(ps))] + ["%r %d %d %d %d" % p for p in ps]
    lines += [str(len(reads))] + [s.decode() or "-" for s in reads]
    path = tmp_path / "in.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    size = int(out[0].split()[1])
    data = np.array(out[1].split()[1:], np.int64)
    res = {}
    for ln in out[2:]:
        t = [int(x) for x in ln.split()[1:]]
        recs = [tuple(t[6 + 7 * i: 13 + 7 * i]) for i in range(t[5])]
        res[t[0], t[1]] = (recs, t[2], t[3], t[4])  # results, satCount, evalCount, evalCount without the stop
    return size, data, res


def digest(per_read):
    return hashlib.sha256(json.dumps(per_read).encode()).hexdigest()


def figures(per_read, full_eval):
    """[reads with a result, reads with >= 2, reads that stopped early, reads with satCount > 0]"""
    return [sum(1 for r in per_read if r[0]), sum(1 for r in per_read if len(r[0]) >= 2),
            sum(1 for r, fe in zip(per_read, full_eval) if r[2] < fe), sum(1 for r in per_read if r[1] > 0)]


@pytest.fixture(scope="module")
def table():
    t = {} if RECORD else load_golden(GOLDEN_FILE)
    yield t
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump(dict(sorted(t.items())), f, indent=1)
            f.write("\n")


def model_results(oracle, cfg, id_bytes, ranks, data, params):
    seeds, h = CFGS[cfg]
    _, _, _, _, reads, prob, minc = make_case(cfg, id_bytes)
    ec, lim, mx, mc, agree = params
    out = []
    for s in reads:
        res, sat, ev = cm.classify(data, ranks, rows_of(oracle, s, seeds, h), id_bytes, bool(seeds), prob, minc,
                                   extra_count=ec, extra_frame_limit=lim, max_miss=mx, min_count=mc, best_hit_agree=bool(agree))
        out.append([[list(map(int, r)) for r in res], int(sat), int(ev)])
    return out


@pytest.mark.parametrize("id_bytes", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("cfg", list(CFGS))
def test_classify_model_against_reference(oracle, driver, table, tmp_path, cfg, id_bytes):
    seeds, h = CFGS[cfg]
    key = "%s_u%d" % (cfg, 8 * id_bytes)
    _, _, entries, occ, reads, _, _ = make_case(cfg, id_bytes)
    assert all(40 <= len(s) <= 120 for s in reads) and any(b"N" in s for s in reads)
    ps = param_sets(bool(seeds))
    live = run_driver(driver, tmp_path, cfg, id_bytes) if driver else None
    size = optimal_size(entries, h, occ)
    if RECORD:
        table[key + "_size"] = live[0]
    assert size == table[key + "_size"]
    ranks, data = build_model_mibf(oracle, cfg, id_bytes, size)
    if live:
        assert live[0] == size and (live[1] == data).all()  # the reference's own ID array
    emptied = 0
    for pi, p in enumerate(ps):
        pkey = key + "_ec%s_lim%d_mm%d_mc%d_agree%d" % p
        got = model_results(oracle, cfg, id_bytes, ranks, data, p)
        if live:
            exp = [[[list(r) for r in live[2][pi, qi][0]], live[2][pi, qi][1], live[2][pi, qi][2]] for qi in range(len(reads))]
            if RECORD:
                table[pkey] = {"sha": digest(exp), "figures": figures(exp, [live[2][pi, qi][3] for qi in range(len(reads))])}
            for qi, (g, e) in enumerate(zip(got, exp)):
                assert g == e, (pkey, qi)
        assert digest(got) == table[pkey]["sha"], pkey
        with_res, multi, early, sat = table[pkey]["figures"]
        print(pkey, table[pkey]["figures"])
        assert with_res * 2 >= len(reads), pkey
        assert multi >= 1 and sat >= 1, pkey
        if p[1] != LARGE:
            assert early >= 1, pkey
        else:
            assert early == 0, pkey
        if p[4]:  # the same set without best_hit_agree comes just before it
            off = model_results(oracle, cfg, id_bytes, ranks, data, ps[pi - 1])
            emptied += sum(1 for a, b in zip(off, got) if len(a[0]) >= 2 and not b[0])
    if RECORD:
        table[key + "_emptied_by_agree"] = emptied
    assert emptied == table[key + "_emptied_by_agree"]


def test_some_read_is_emptied_by_best_hit_agree(table):
    """after the cases above (which fill the table when recording)"""
    assert sum(v for k, v in table.items() if k.endswith("_emptied_by_agree")) >= 1
