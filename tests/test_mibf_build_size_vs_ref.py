"""btlbf_mibf_optimal_size against the genuine reference over entries {1, 63, 16000, 1.2e9, 2^40} x h {1, 4, 8} x
occupancy {0.1, 0.3, 0.5, 0.9}.

Where the reference is built (oracle/_ref, the `ref` fixture) the size is the genuine constructor's filter_size()
(MIBFConstructSupport's, through ref.mibf) for every grid point whose bit vector the constructor can allocate -- it
allocates what it sizes, so 1.2e9 and 2^40 entries (up to 10^13 bits) cannot be asked of it -- and, for EVERY grid point,
the genuine static MIBloomFilter<T>::calcOptimalSize, the function that constructor calls (MIBFConstructSupport.hpp:43),
through tests/cpp/ref_mibf_optimal_size_driver.cpp.  The values are recorded in tests/golden/mibf_optimal_size_vs_ref.json
(BTLBF_RECORD_REF_GOLDEN=1 python -m pytest tests/test_mibf_build_size_vs_ref.py, where the reference lies), so that a
machine without the reference checks the library against the same numbers."""
import json
import os
import subprocess

import pytest
from conftest import GOLDEN, ROOT, load_golden

GOLDEN_FILE = "mibf_optimal_size_vs_ref.json"
RECORD = bool(os.environ.get("BTLBF_RECORD_REF_GOLDEN"))
REF_DIR = os.environ.get("BTLBF_REFERENCE_DIR", "/root/reference")
GRID = [(e, h, occ) for e in (1, 63, 16000, 1200000000, 1 << 40) for h in (1, 4, 8) for occ in (0.1, 0.3, 0.5, 0.9)]
CONSTRUCTIBLE = 1 << 28  # bits the constructor is asked to allocate at the most (32 MiB)


def key(e, h, occ):
    return "%d_%d_%r" % (e, h, occ)


def test_optimal_size_equals_the_recorded_reference_values(lib):
    table = load_golden(GOLDEN_FILE)
    assert sorted(table) == sorted(key(*g) for g in GRID)
    for e, h, occ in GRID:
        assert lib.btlbf_mibf_optimal_size(e, h, occ) == table[key(e, h, occ)], (e, h, occ)
        assert table[key(e, h, occ)] % 64 == 0


def test_optimal_size_equals_the_genuine_constructor(lib, ref):
    """skips where the reference is not built, as the other *_vs_ref tests do"""
    if not ref.has_mibf():
        pytest.skip("oracle/_ref was built before the miBF driver existed")
    table = load_golden(GOLDEN_FILE)
    asked = 0
    for e, h, occ in GRID:
        got = lib.btlbf_mibf_optimal_size(e, h, occ)
        if got > CONSTRUCTIBLE:
            continue
        r = ref.mibf(2, e, 31, h, occ)
        size = r.filter_size()
        r.insert_bv(b"ACGTTGCAAGCTTCGAGGATCCATATGCTAGCAAGGTT")  # the driver's teardown runs the later stages: not on no bit
        r.close()
        assert got == size == table[key(e, h, occ)], (e, h, occ)
        asked += 1
    assert asked == 3 * 3 * 4  # every point of 1, 63 and 16000 entries


def test_optimal_size_equals_the_genuine_static_function(lib, tmp_path):
    if not os.path.exists(os.path.join(REF_DIR, "MIBloomFilter.hpp")):
        if RECORD:
            pytest.fail("recording needs the reference tree")
        pytest.skip("no reference tree on this machine")
    exe = str(tmp_path / "ref_mibf_optimal_size_driver")
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-w", "-I" + REF_DIR,
                        "-I" + os.path.join(ROOT, "oracle", "standin"), "-I" + os.path.join(ROOT, "tests", "cpp", "standin"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_mibf_optimal_size_driver.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args = [x for e, h, occ in GRID for x in (str(e), str(h), repr(occ))]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = [int(x) for x in r.stdout.split()]
    assert len(sizes) == len(GRID)
    if RECORD:
        with open(os.path.join(GOLDEN, GOLDEN_FILE), "w") as f:
            json.dump({key(*g): s for g, s in zip(GRID, sizes)}, f, indent=1, sort_keys=True)
            f.write("\n")
    table = load_golden(GOLDEN_FILE)
    for (e, h, occ), s in zip(GRID, sizes):
        assert lib.btlbf_mibf_optimal_size(e, h, occ) == s == table[key(e, h, occ)], (e, h, occ)
