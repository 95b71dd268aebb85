"""The C++ layer over the filter algebra: tests/cpp/test_algebra_shim.cpp (BloomFilter::merge / intersect / subtract /
fold, CountingBloomFilter<T>::merge / fold / toBloomFilter on stored filters, every identity checked with btlbf_compare)
and examples/bloom_merge.cpp (union, fold and solid over stored files, whose results must load and equal the filters
Python builds from the same reads)."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_gpu_auto_query import bf  # noqa: F401  (fixture)
from test_gpu_cpp_screen import build_program

H, K, L = 3, 25, 100
BITS = 1 << 18


@pytest.fixture(scope="module")
def stored(bf, tmp_path_factory):  # noqa: F811
    """bit and counting (8-bit, incrementAll, one read five times) filters of reads R1, R2 and both, at two sizes"""
    import torch

    tmp = tmp_path_factory.mktemp("cppalgebra")
    r1 = torch.cat([bf.synth_reads_device(5, 0, 200, L)] + [bf.synth_reads_device(6, 0, 1, L)] * 5)
    r2 = bf.synth_reads_device(7, 0, 150, L)
    paths, filters = {}, {}
    for name, reads, bits in (("a", r1, BITS), ("b", r2, BITS), ("both", torch.cat([r1, r2]), BITS),
                              ("both_half", torch.cat([r1, r2]), BITS // 2)):
        f = bf.BloomFilter(bits, H, K)
        f.insertSeqs(reads, read_len=L)
        c = bf.CountingBloomFilter(bits // 8, H, K, countThreshold=2)
        c.insertSeqs(reads, read_len=L, increment_all=True)
        for tag, x in (("", f), ("c", c)):
            paths[tag + name] = str(tmp / (tag + name + ".bf"))
            x.storeFilter(paths[tag + name])
            filters[tag + name] = x
    return bf, tmp, paths, filters


@pytest.mark.gpu
def test_shim_members(stored, tmp_path):
    bf, _, paths, filters = stored  # noqa: F811
    exe = build_program(tmp_path, os.path.join("tests", "cpp", "test_algebra_shim.cpp"))
    names = ["a", "b", "both", "both_half", "ca", "cb", "cboth", "cboth_half"]
    r = subprocess.run([exe] + [paths[n] for n in names], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "algebra shim ok" in r.stdout, r.stdout + r.stderr
    out = dict(ln.split() for ln in r.stdout.splitlines() if " " in ln and not ln.startswith("algebra"))
    assert int(out["union_pop"]) == filters["both"].getPop()
    assert int(out["fold_pop"]) == filters["both_half"].getPop()
    assert int(out["solid_pop"]) == filters["cboth"].filtered_popcount() > 0


@pytest.mark.gpu
def test_bloom_merge_round_trip(stored, tmp_path):
    bf, _, paths, filters = stored  # noqa: F811
    exe = build_program(tmp_path, os.path.join("examples", "bloom_merge.cpp"))

    def run(*args):
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    out = str(tmp_path / "union.bf")
    text = run("union", out, paths["a"], paths["b"])
    u = bf.BloomFilter(path=out)
    assert u.compare(filters["both"]) == (0, 0, 0) and u.header() == filters["both"].header()
    assert "set %d" % filters["both"].getPop() in text
    out = str(tmp_path / "half.bf")
    run("fold", "2", out, paths["both"])
    assert bf.BloomFilter(path=out).compare(filters["both_half"]) == (0, 0, 0)
    out = str(tmp_path / "solid.bf")
    run("solid", "2", out, paths["cboth"])
    s = bf.BloomFilter(path=out)
    assert s.compare(filters["cboth"].toBloomFilter(2)) == (0, 0, 0) and s.getPop() == filters["cboth"].filtered_popcount()
    out = str(tmp_path / "common.bf")
    run("intersect", out, paths["both"], paths["a"])
    assert bf.BloomFilter(path=out).compare(filters["a"]) == (0, 0, 0)
    r = subprocess.run([exe, "fold", "3", out, paths["both"]], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "does not divide" in r.stderr
