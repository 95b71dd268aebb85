"""The C++ layer over the read screen: tests/cpp/test_screen_shim.cpp (btlbf::ReadScreen: screen, screenFile through a
functor, summarizeFile, on two stored filters) and examples/bloom_screen.cpp (two stored filters and a gzipped FASTQ)
against the Python layer on the same files.  (That both programs compile without a GPU is checked by
tests/test_screen_abi_cpu.py.)"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import screen_cases as sc
from conftest import ROOT
from screen_model import tally_model
from test_gpu_auto_query import bf  # noqa: F401  (fixture)


def build_program(tmp_path, source):
    from btl_bloomfilter_amd import build

    build.build()
    exe = str(tmp_path / os.path.splitext(os.path.basename(source))[0])
    lib_dir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, source),
                        "-L" + lib_dir, "-lbtlbf", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def stored(bf, tmp_path_factory):  # noqa: F811
    """two stored filters, 300 reads as FASTQ (plain and gzipped), and what Python computes on them"""
    tmp = tmp_path_factory.mktemp("cppscreen")
    rng = np.random.RandomState(77)
    genome = [sc.random_bases(rng, 8000) for _ in range(2)]
    reads = []
    for i in range(300):
        n = [0, 20, 31, 100, 150, 151][i % 6]
        if i % 2 and n:
            o = rng.randint(0, 8000 - n)
            reads.append(genome[(i // 2) % 2][o:o + n].copy())
        else:
            reads.append(sc.random_bases(rng, n))
    paths = []
    filters = []
    for j, (bits, g) in enumerate(zip((1 << 17, 100000), genome)):
        f = bf.BloomFilter(bits, 4, 31)
        f.insertSeqs(g)
        paths.append(str(tmp / ("f%d.bf" % j)))
        f.storeFilter(paths[-1])
        filters.append(f)
    fq = str(tmp / "reads.fq")
    open(fq, "wb").write(sc.fastq_bytes(reads))
    with gzip.open(fq + ".gz", "wb") as z:
        z.write(open(fq, "rb").read())
    buf = np.concatenate(reads)
    starts = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    exp = bf.screenSeqs(filters, buf, starts=starts, min_fraction=0.5, min_hits=2)
    return bf, paths, fq, reads, exp


@pytest.mark.gpu
def test_shim_members_against_python(stored, tmp_path):
    bf, paths, fq, reads, exp = stored
    exe = build_program(tmp_path, os.path.join("tests", "cpp", "test_screen_shim.cpp"))
    r = subprocess.run([exe, paths[0], paths[1], fq, "0.5", "2", "5000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    want = [[i, int(exp[0][i, 0]), int(exp[0][i, 1]), int(exp[1][i]), int(exp[2][i])] for i in range(len(reads))]
    for tag in ("mem", "file"):
        got = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == tag]
        assert got == want, tag
    out = {ln[0]: ln[1:] for ln in lines if ln[0] not in ("mem", "file")}
    assert out["file_rows"][0] == "300" and int(out["file_rows"][1]) >= 5 and out["file_rows"][2] == "1"
    passed, best, totals = tally_model(*exp)
    assert [int(x) for x in out["passed"]] == passed.tolist() and [int(x) for x in out["best"]] == best.tolist()
    assert [int(x) for x in out["totals"]] == totals.tolist() and passed.sum() > 50 and totals[1] > 50
    assert [int(x) for x in out["stats"]] == [300, sum(r.size for r in reads), int(exp[1].sum())]
    assert out["refused"][0] == "1" and "twice" in " ".join(out["refused"])


@pytest.mark.gpu
def test_example_on_two_stored_filters_and_a_gzipped_fastq(stored, tmp_path):
    bf, paths, fq, reads, exp = stored
    exe = build_program(tmp_path, os.path.join("examples", "bloom_screen.cpp"))
    r = subprocess.run([exe, "-s", "0.5", "-m", "2", "-b", "5000", fq + ".gz", paths[0], paths[1]], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    passed, best, totals = tally_model(*exp)
    lines = r.stdout.splitlines()
    assert lines[:2] == ["%s\t%d\t%d" % (paths[j], passed[j], best[j]) for j in range(2)]
    assert lines[2] == "#totals\treads %d\tpassing none %d\tpassing several %d\twithout a k-mer %d\tk-mers %d" % (
        *totals.tolist(), int(exp[1].sum()))
    r = subprocess.run([exe, fq], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
