"""examples/mibf_build.cpp, and examples/mibf_classify.cpp on what it writes: the example's .bf and .mibf equal the files
the Python layer stores after buildFromFiles on the same inputs byte for byte, the .ids.tsv is checked line by line, and
mibf_classify on the example's files prints the rows classifyFile gives.  (That the example compiles and refuses without a
GPU is checked by tests/test_mibf_build_abi_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_mibf_classify_file import build_program
from test_gpu_mibf_build_file import World
from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)
from test_gpu_mibf_classify_file import fastq
from test_mibf_classify_vs_ref import K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(bf, tmp_path_factory):  # noqa: F811
    return World(bf, "C5", 2, tmp_path_factory.mktemp("cppbuild"))


def run_example(exe, prefix, w, *options):
    r = subprocess.run([exe, prefix, str(K), repr(w.occ)] + w.paths + ["--seeds", ",".join(w.seeds), "--bits", str(w.bits),
                                                                     "--batch-bytes", "1100"] + list(options),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(ln.split("\t", 1) for ln in r.stdout.splitlines())


@pytest.mark.parametrize("per_record", [True, False], ids=["per_record", "per_file"])
def test_example_writes_the_python_files_and_the_id_table(world, tmp_path, per_record):
    w = world
    exe = build_program(tmp_path, os.path.join("examples", "mibf_build.cpp"))
    prefix = str(tmp_path / "cpp")
    out = run_example(exe, prefix, w, "--serial", "--first-id", "3", *(["--per-record"] if per_record else []))
    m, f, rep = w.build(ids="record" if per_record else "file", first_id=3, saturation="serial", batch_bytes=1100)
    f.storeFilter(str(tmp_path / "py.bf"))
    m.store(str(tmp_path / "py.mibf"))
    for ext in (".bf", ".mibf"):
        assert open(prefix + ext, "rb").read() == open(str(tmp_path / "py") + ext, "rb").read(), ext
    n_ids = len(w.S) if per_record else 3
    assert out["records"] == str(len(w.S)) and out["ids"] == str(n_ids) and out["table size"] == str(3 + n_ids)
    assert out["bits"] == str(w.bits) and out["pop"] == str(m.getPop()) and out["longest record"] == "350"
    assert out["saturation"] == "clean %d\tfound %d\tmutated %d\tsaturated %d" % tuple(rep["sat_counts4"])
    lines = open(prefix + ".ids.tsv").read().splitlines()
    if per_record:
        exp = ["%d\t%s\t%d" % (3 + sum(w.per_file[:j]) + r, w.paths[j], r) for j in range(3) for r in range(w.per_file[j])]
    else:
        exp = ["%d\t%s" % (3 + j, w.paths[j]) for j in range(3)]
    assert lines == exp


def test_build_then_classify_end_to_end(world, tmp_path):
    w = world
    build = build_program(tmp_path, os.path.join("examples", "mibf_build.cpp"))
    classify = build_program(tmp_path, os.path.join("examples", "mibf_classify.cpp"))
    prefix = str(tmp_path / "refs")
    out = run_example(build, prefix, w, "--per-record", "--scratch-bytes", str(1 << 20))  # parallel saturation
    n_ids = int(out["table size"])
    assert n_ids == 1 + len(w.S)
    reads = fastq(tmp_path / "reads.fq", [np.frombuffer(s, np.uint8) for s in w.reads])
    r = subprocess.run([classify, prefix + ".bf", prefix + ".mibf", str(n_ids), reads, "--max-miss", "1",
                        "--extra-frame-limit", "2", "--max-results", "3", "--batch-bytes", "400"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(x) for x in ln.split("\t")) for ln in r.stdout.splitlines() if not ln.startswith("#")]
    m, _, _ = w.build(ids="record", first_id=1, saturation="parallel", batch_bytes=1100, scratch_bytes=1 << 20)
    prob, _ = m.calcFrameProbs(n_ids, 1)
    exp = []
    for first, hits, n, sat, ev in m.classifyFile(reads, prob, [1] * n_ids, max_miss=1, extra_frame_limit=2, max_results=3,
                                                  batch_bytes=400):
        for i in range(len(n)):
            exp += [(first + i, int(h["id"]), int(h["count"]), int(h["nonSatFrameCount"])) for h in hits[i, :min(n[i], 3)]]
    assert got == exp and len({g[0] for g in got}) * 3 >= len(w.reads)
    assert r.stdout.splitlines()[-1].startswith("#totals\trows %d\t" % len(w.reads))
