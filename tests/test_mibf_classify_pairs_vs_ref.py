"""The paired classification model -- tests/mibf_classify_model.py::classify over the two mates' rows interleaved, the
checker of tests/test_gpu_mibf_classify_pairs.py -- against the genuine reference: MIBFQuerySupport<T>::query(itr1, itr2,
minCount) (MIBFQuerySupport.hpp:111-130) compiled behind tests/cpp/ref_mibf_classify_pair_driver.cpp, as
tests/test_mibf_classify_vs_ref.py does for single reads (same stand-ins, same miBF, same parameter sets).

The reference's outputs on these seeded pairs are pinned in tests/golden/mibf_classify_pairs_vs_ref.json (a digest per
parameter set and the figures the conditions below are asserted on), so the test runs everywhere; where the reference
tree is present the driver is built and compared live as well.  The pins were recorded from the reference build, never
from the model, with
    BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_mibf_classify_pairs_vs_ref.py

Conditions on the reference's own output, so that no case passes vacuously.  Per parameter set: at least a third of the
pairs have a result; with extra_frame_limit 0 or 2 at least one pair stops early (its evalCount below that of the same
query without the stop) and with the large limit none does; with limit 0 or 2 the model over the CONCATENATED rows (all
of mate 1, then all of mate 2) differs from the reference's paired result for at least one pair -- a walk in the wrong
frame order cannot pass.  Per configuration, over all its sets: one pair has two results and one has satCount > 0."""
import json
import os
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, load_golden

import mibf_classify_model as cm
import test_mibf_classify_vs_ref as cr
from test_mibf_classify_vs_ref import CFGS, K, LARGE, REF_DIR, build_model_mibf, digest, make_case, optimal_size, param_sets, rows_of

GOLDEN_FILE = "mibf_classify_pairs_vs_ref.json"
RECORD = cr.RECORD
PAIR_SEED = 1000


def make_pairs(cfg, id_bytes):
    """20 pairs (mate 1, mate 2) of bytes on the genomes of make_case: 16 seeded ones of four kinds in turn, mates of
    40..120 bases, then four fixed ones (a mate shorter than k, an empty mate, both empty, an all-N mate 1 with a
    single-frame mate 2)"""
    genomes = [np.frombuffer(g, np.uint8) for g in make_case(cfg, id_bytes)[0]]
    rng = np.random.RandomState(PAIR_SEED)
    n = len(genomes)
    pairs = []
    for r in range(16):
        i = rng.randint(0, n)
        g = genomes[i]
        n1, n2 = rng.randint(40, 121), rng.randint(40, 121)
        if r % 4 == 0:  # mate 1 in the ID's own 150 bases, mate 2 from base 150 on (the part it shares, and behind it)
            o1, o2 = rng.randint(0, 150 - n1 + 1), rng.randint(150, g.size - n2 + 1)
            m1, m2 = g[o1:o1 + n1], g[o2:o2 + n2]
        elif r % 4 == 1:  # the mates come from two IDs
            m1, m2 = g[:n1], genomes[(i + 3) % n][200:200 + n2]
        elif r % 4 == 2:  # mate 1 of a few frames only
            n1 = K + rng.randint(0, 6)
            o1, o2 = rng.randint(0, g.size - n1 + 1), rng.randint(0, g.size - n2 + 1)
            m1, m2 = g[o1:o1 + n1], g[o2:o2 + n2]
        else:  # both anywhere in one genome
            o1, o2 = rng.randint(0, g.size - n1 + 1), rng.randint(0, g.size - n2 + 1)
            m1, m2 = g[o1:o1 + n1], g[o2:o2 + n2]
        m1, m2 = m1.copy(), m2.copy()
        if r % 5 == 0:
            m1[rng.randint(0, m1.size)] = ord("N")
        if r % 5 == 1:
            m2[rng.randint(0, m2.size)] = ord("N")
        pairs.append((m1.tobytes(), m2.tobytes()))
    g0 = genomes[0].tobytes()
    pairs += [(g0[:K - 1], g0[160:240]), (g0[160:240], b""), (b"", b""), (b"N" * 50, g0[5:5 + K])]
    return pairs


def interleave(rows1, rows2):
    """the frame sequence of a pair (MIBFQuerySupport.hpp:120-126): at an even frameCount mate 1's next frame if it has
    one, else mate 2's; at an odd frameCount mate 2's if it has one, else mate 1's"""
    out, i, j = [], 0, 0
    while i < len(rows1) or j < len(rows2):
        if (len(out) % 2 == 0 and i < len(rows1)) or j >= len(rows2):
            out.append(rows1[i])
            i += 1
        else:
            out.append(rows2[j])
            j += 1
    return np.array(out, np.uint64).reshape(len(out), rows1.shape[1])


def pair_rows(oracle, cfg, m1, m2):
    seeds, h = CFGS[cfg]
    empty = np.zeros((0, h), np.uint64)
    return (rows_of(oracle, m1, seeds, h) if m1 else empty), (rows_of(oracle, m2, seeds, h) if m2 else empty)


def model_pairs(oracle, cfg, id_bytes, ranks, data, params, order=interleave):
    """[[records], satCount, evalCount] per pair; order: how the two mates' rows become one frame sequence"""
    seeds, h = CFGS[cfg]
    _, _, _, _, _, prob, minc = make_case(cfg, id_bytes)
    ec, lim, mx, mc, agree = params
    out = []
    for m1, m2 in make_pairs(cfg, id_bytes):
        r1, r2 = pair_rows(oracle, cfg, m1, m2)
        res, sat, ev = cm.classify(data, ranks, order(r1, r2), id_bytes, bool(seeds), prob, minc, extra_count=ec,
                                   extra_frame_limit=lim, max_miss=mx, min_count=mc, best_hit_agree=bool(agree))
        out.append([[list(map(int, r)) for r in res], int(sat), int(ev)])
    return out


def concatenated(rows1, rows2):
    return np.concatenate([rows1, rows2])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the reference driver, built where the reference tree lies; None elsewhere"""
    if not os.path.exists(os.path.join(REF_DIR, "MIBFQuerySupport.hpp")):
        if RECORD:
            pytest.fail("recording needs the reference tree")
        return None
    exe = str(tmp_path_factory.mktemp("refclsp") / "ref_mibf_classify_pair_driver")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-w", "-fno-access-control", "-I" + REF_DIR,
                        "-I" + os.path.join(ROOT, "oracle", "standin"), "-I" + os.path.join(ROOT, "tests", "cpp", "standin"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_mibf_classify_pair_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_pair_driver(exe, tmp_path, monkeypatch, cfg, id_bytes):
    """run_driver of the single-read test on the mates as its queries -> (size, data, {(p, pair): results})"""
    mates = [m for pair in make_pairs(cfg, id_bytes) for m in pair]
    case = make_case(cfg, id_bytes)
    monkeypatch.setattr(cr, "make_case", lambda c, b: case[:4] + (mates,) + case[5:])
    return cr.run_driver(exe, tmp_path, cfg, id_bytes)


@pytest.fixture(scope="module")
def table():
    t = {} if RECORD else load_golden(GOLDEN_FILE)
    yield t
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump(dict(sorted(t.items())), f, indent=1)
            f.write("\n")


def test_interleave_is_the_reference_order():
    a, b = np.arange(10, 13, dtype=np.uint64).reshape(3, 1), np.arange(20, 25, dtype=np.uint64).reshape(5, 1)
    assert interleave(a, b).ravel().tolist() == [10, 20, 11, 21, 12, 22, 23, 24]
    assert interleave(b, a).ravel().tolist() == [20, 10, 21, 11, 22, 12, 23, 24]
    assert interleave(a[:0], b).ravel().tolist() == [20, 21, 22, 23, 24] and interleave(a, b[:0]).ravel().tolist() == [10, 11, 12]
    assert interleave(a[:0], b[:0]).shape == (0, 1)


@pytest.mark.parametrize("id_bytes", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("cfg", list(CFGS))
def test_paired_model_against_reference(oracle, driver, table, tmp_path, monkeypatch, cfg, id_bytes):
    seeds, h = CFGS[cfg]
    key = "%s_u%d" % (cfg, 8 * id_bytes)
    _, _, entries, occ, _, _, _ = make_case(cfg, id_bytes)
    pairs = make_pairs(cfg, id_bytes)
    assert len(pairs) == 20 and all(40 <= len(m) <= 120 for p in pairs[:16] for m in p if len(m) > K + 5)
    ps = param_sets(bool(seeds))
    size = optimal_size(entries, h, occ)
    ranks, data = build_model_mibf(oracle, cfg, id_bytes, size)
    live = run_pair_driver(driver, tmp_path, monkeypatch, cfg, id_bytes) if driver else None
    if live:
        assert live[0] == size and (live[1] == data).all()  # the reference's own ID array
    multi = sat = 0
    for pi, p in enumerate(ps):
        pkey = key + "_ec%s_lim%d_mm%d_mc%d_agree%d" % p
        got = model_pairs(oracle, cfg, id_bytes, ranks, data, p)
        if live:
            exp = [[[list(r) for r in live[2][pi, qi][0]], live[2][pi, qi][1], live[2][pi, qi][2]] for qi in range(len(pairs))]
            if RECORD:
                cat = model_pairs(oracle, cfg, id_bytes, ranks, data, p, order=concatenated)
                table[pkey] = {"sha": digest(exp),
                               "figures": cr.figures(exp, [live[2][pi, qi][3] for qi in range(len(pairs))]),
                               "concatenation_differs": sum(1 for c, e in zip(cat, exp) if c != e)}
            for qi, (g, e) in enumerate(zip(got, exp)):
                assert g == e, (pkey, qi)
        assert digest(got) == table[pkey]["sha"], pkey
        with_res, two, early, with_sat = table[pkey]["figures"]
        print(pkey, table[pkey]["figures"], table[pkey]["concatenation_differs"])
        assert with_res * 3 >= len(pairs), pkey
        if p[1] != LARGE:
            assert early >= 1, pkey
            # got equals the reference's result (the digest above), so this is the reference against concatenation
            cat = model_pairs(oracle, cfg, id_bytes, ranks, data, p, order=concatenated)
            differs = sum(1 for c, g in zip(cat, got) if c != g)
            assert differs == table[pkey]["concatenation_differs"] and differs >= 1, pkey
        else:
            assert early == 0, pkey
        multi += two
        sat += with_sat
    assert multi >= 1 and sat >= 1, key
