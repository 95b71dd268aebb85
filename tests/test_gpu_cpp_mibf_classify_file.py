"""The C++ layer over the file classifier: examples/mibf_classify.cpp (loads a stage-1 .bf and a miBF data file, calls
calcFrameProbs, classifies two FASTQ files and prints a line per result) and tests/cpp/test_mibf_file_shim.cpp
(calcFrameProbs, summarizeFile, queryFiles / queryInterleavedFile / queryFile through functors) against the Python layer
on the same files.  (That both programs compile without a GPU is checked by tests/test_mibf_classify_file_abi_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mibf_tally_model import tally_model
from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)
from test_gpu_mibf_classify_file import Files, fastq  # noqa: F401

MAX_MISS = 1


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
    """the miBF of the file tests stored as the two files a C++ caller loads, and what Python computes on them"""
    tmp = tmp_path_factory.mktemp("cppfile")
    files = Files(bf, tmp)
    c = files.case
    stage1, data = str(tmp / "stage1.bf"), str(tmp / "ids.mibf")
    f = bf.BloomFilter(c.m.size(), c.h, 31)
    f.setSpacedSeeds(c.seeds, 1)
    seq = np.concatenate(c.genomes)
    f.insertSeqs(seq, starts=np.concatenate([[0], np.cumsum([g.size for g in c.genomes])]).astype(np.uint64))
    f.storeFilter(stage1)
    f.close()
    c.m.store(data)
    prob, sat_prop = c.m.calcFrameProbs(c.n_ids, MAX_MISS)
    return files, stage1, data, prob, sat_prop


@pytest.mark.gpu
def test_example_prints_the_python_rows(stored, tmp_path):
    files, stage1, data, prob, _ = stored
    c = files.case
    exe = build_program(tmp_path, os.path.join("examples", "mibf_classify.cpp"))
    r = subprocess.run([exe, stage1, data, str(c.n_ids), files.f1, files.f2, "--max-miss", str(MAX_MISS),
                        "--extra-frame-limit", "2", "--max-results", "3", "--batch-bytes", "300"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    minc = [1] * c.n_ids
    exp_rows, best, any_ = [], np.zeros(c.n_ids, np.uint64), np.zeros(c.n_ids, np.uint64)
    n_rows = without = 0
    it = c.m.classifyFile(files.f1, prob, minc, path2=files.f2, max_miss=MAX_MISS, extra_frame_limit=2, max_results=3,
                          batch_bytes=300)
    for first, hits, n, sat, ev in it:
        for i in range(len(n)):
            without += n[i] == 0
            exp_rows += [(first + i, int(h["id"]), int(h["count"]), int(h["nonSatFrameCount"])) for h in hits[i, :min(n[i], 3)]]
        n_rows += len(n)
    best, any_, totals = it.tally()
    lines = r.stdout.splitlines()
    got_rows = [tuple(int(x) for x in ln.split("\t")) for ln in lines if not ln.startswith("#")]
    assert n_rows == 20 and len(exp_rows) >= 20 and got_rows == exp_rows
    got_ids = {int(ln[1:].split("\t")[0]): tuple(int(x) for x in ln.split("\t")[1:]) for ln in lines
               if ln.startswith("#") and not ln.startswith("#totals")}
    assert got_ids == {i: (int(best[i]), int(any_[i])) for i in range(c.n_ids) if any_[i]}
    assert lines[-1].startswith("#totals\trows 20\twithout a result %d\t" % without) and totals[1] == without


@pytest.mark.gpu
def test_shim_members_against_python(stored, tmp_path):
    files, stage1, data, prob, sat_prop = stored
    c = files.case
    exe = build_program(tmp_path, os.path.join("tests", "cpp", "test_mibf_file_shim.cpp"))
    r = subprocess.run([exe, stage1, data, str(c.n_ids), str(MAX_MISS), files.f1, files.f2, files.il],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    got = [float.fromhex(x) for x in out["probs"]]
    assert got[0] == sat_prop and got[1] == -1.0 and got[2:] == [float(x) for x in prob[1:]]  # entry 0 untouched
    assert float.fromhex(out["single"][0]) == c.m.calcProbSingleFrame(0.25, 4, 0.125, 1)
    p0 = prob.copy()
    p0[0] = 0.0
    kw = dict(max_miss=MAX_MISS, extra_frame_limit=2, max_results=3, batch_bytes=300)
    minc = [1] * c.n_ids
    best, any_, totals = c.m.classifyFile(files.f1, p0, minc, path2=files.f2, summary_only=True, **kw)
    assert [int(x) for x in out["best"]] == best.tolist() and [int(x) for x in out["any"]] == any_.tolist()
    assert [int(x) for x in out["totals"]] == totals.tolist() and totals[0] == 20
    seq, starts = files.case.bf.interleave_mates(files.m1, files.m2)
    mem = c.m.classifyPairs(seq, p0, minc, starts=starts, max_miss=MAX_MISS, extra_frame_limit=2, max_results=3)
    assert [x.tolist() for x in tally_model(*mem, c.n_ids, 3)] == [best.tolist(), any_.tolist(), totals.tolist()]

    def checksum(rows):
        s = 0
        for hits, n, sat, ev in rows:
            s = (s * 1000003 + int(sat) * 31 + int(ev)) % 2**64
            for h in hits[:min(int(n), 3)]:
                s = (s * 1000003 + int(h["id"]) + 7 * int(h["count"]) + 11 * int(h["nonSatCount"]) + 13 * int(h["totalCount"])
                     + 17 * int(h["totalNonSatCount"]) + 19 * int(h["nonSatFrameCount"]) + 23 * int(h["solidCount"])) % 2**64
        return s

    exp = checksum(zip(*mem))
    assert out["two"] == ["20", "1", str(exp)] and out["interleaved"] == ["20", "1", str(exp)]
    assert out["single_rows"] == ["40", "1"]

