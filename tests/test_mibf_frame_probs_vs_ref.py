"""calcFrameProbs: the Python restatement tests/mibf_frame_probs_model.py (the checker of btlbf_mibf_frame_probs in
tests/test_gpu_mibf_frame_probs.py) against the genuine reference, MIBloomFilter<T>::calcFrameProbs compiled behind
tests/cpp/ref_mibf_frame_probs_driver.cpp over the stand-ins of oracle/standin/ and tests/cpp/standin/, on the miBF of
make_case for every configuration and id type and every allowedMiss 0..h-1.

Where the reference tree is present the driver is built and the model must equal it BIT FOR BIT (same machine, same libm:
math.pow is the C library's pow).  The reference's values are pinned as hex floats in
tests/golden/mibf_frame_probs_vs_ref.json -- recorded from the reference build, never from the model, with
    BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_mibf_frame_probs_vs_ref.py
-- so the test runs everywhere; against the pins the model is held to a relative 1e-11: another libm's pow may differ by
an ulp, and 1 - pow(1 - freq, i) amplifies a relative error of its argument by 1 / freq.  With every id's share of the
entries at least 1/1024 that is 2^10 * ~8 * 2^-53 ~ 9e-13.  Both conditions of that bound are asserted (the shares, and
that the probabilities differ between ids, so that a constant cannot pass)."""
import json
import os
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, load_golden

from mibf_frame_probs_model import frame_probs_model, sat_prop_model
from test_mibf_classify_vs_ref import CFGS, K, REF_DIR, build_model_mibf, make_case, optimal_size

GOLDEN_FILE = "mibf_frame_probs_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))
REL = 1e-11


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the reference driver, built where the reference tree lies; None elsewhere"""
    if not os.path.exists(os.path.join(REF_DIR, "MIBloomFilter.hpp")):
        if RECORD:
            pytest.fail("recording needs the reference tree")
        return None
    exe = str(tmp_path_factory.mktemp("refprobs") / "ref_mibf_frame_probs_driver")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-w", "-fno-access-control", "-I" + REF_DIR,
                        "-I" + os.path.join(ROOT, "oracle", "standin"), "-I" + os.path.join(ROOT, "tests", "cpp", "standin"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_mibf_frame_probs_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, tmp_path, cfg, id_bytes, n_bins):
    seeds, h = CFGS[cfg]
    seqs, ids, entries, occ, _, _, _ = make_case(cfg, id_bytes)
    lines = ["%d %d %d %d %s %d %r" % (id_bytes, K, h, len(seeds or ()), " ".join(seeds or ()), entries, occ), str(len(seqs))]
    lines += ["%d %s" % (i, s.decode()) for i, s in zip(ids, seqs)] + [str(n_bins)]
    path = tmp_path / "in.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    size, pop = (int(x) for x in out[0].split()[1:])
    counts = [int(x) for x in out[1].split()[1:]]
    probs = {int(ln.split()[1]): ln.split()[2:] for ln in out[2:]}
    return {"size": size, "pop": pop, "saturated": counts[0], "counts": counts[1:],
            "probs": {str(a): v for a, v in sorted(probs.items())}}


@pytest.fixture(scope="module")
def table():
    t = {} if RECORD else load_golden(GOLDEN_FILE)
    yield t
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump(dict(sorted(t.items())), f, indent=1)
            f.write("\n")


def id_counts(data, id_bytes, n_bins):
    """getIDCounts (MIBloomFilter.hpp:539-551) over the model's data array"""
    mask = 1 << (8 * id_bytes - 1)
    v = np.asarray(data, np.int64)
    sat = v > mask
    return np.bincount(np.where(sat, v & (mask - 1), v), minlength=n_bins).tolist(), int(sat.sum())


@pytest.mark.parametrize("id_bytes", [2, 4], ids=["u16", "u32"])
@pytest.mark.parametrize("cfg", list(CFGS))
def test_frame_probs_model_against_reference(oracle, driver, table, tmp_path, cfg, id_bytes):
    seeds, h = CFGS[cfg]
    key = "%s_u%d" % (cfg, 8 * id_bytes)
    _, ids, entries, occ, _, _, _ = make_case(cfg, id_bytes)
    n_bins = int(max(ids)) + 1
    live = run_driver(driver, tmp_path, cfg, id_bytes, n_bins) if driver else None
    if RECORD:
        table[key] = live
    pin = table[key]
    size = optimal_size(entries, h, occ)
    assert size == pin["size"] and sorted(pin["probs"]) == [str(a) for a in range(h)]
    # the model's miBF (pinned to the reference's by test_mibf_vs_ref.py) gives the reference's counts
    ranks, data = build_model_mibf(oracle, cfg, id_bytes, size)
    counts, saturated = id_counts(data, id_bytes, n_bins)
    assert len(counts) == n_bins and (ranks.pop, saturated, counts) == (pin["pop"], pin["saturated"], pin["counts"])
    # the two conditions of the 1e-11 bound
    total = sum(counts[1:])
    assert all(c * 1024 >= total for c in counts[1:]), "an id holds less than 1/1024 of the entries"
    for a in range(h):
        got = frame_probs_model(counts, ranks.pop, size, h, a)
        got = [sat_prop_model(counts, saturated)] + got[1:]
        exp = [float.fromhex(x) for x in pin["probs"][str(a)]]
        assert len(got) == len(exp) == n_bins
        assert len(set(exp[1:])) >= 2, "every id has the same probability"
        print(key, a, "max rel", max(abs(g - e) / e for g, e in zip(got, exp)))
        assert all(e > 0 and abs(g - e) <= REL * e for g, e in zip(got, exp)), (key, a)
        if live:  # same machine, same libm: bit for bit
            assert [g.hex() for g in got] == [float.fromhex(x).hex() for x in live["probs"][str(a)]], (key, a)
