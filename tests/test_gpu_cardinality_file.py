"""The k-mer cardinality sketch over FASTA / FASTQ files (btlbf_card_add_fastx through KmerCardinality.addFile): the
sketch of a file equals the sketch of the same records added from memory -- FASTQ plain and gzipped, wrapped FASTA as
records and line by line; with batches of a few KiB the file rotates through both device slots and records are cut at
batch ends (the parser's k - 1 base overlap), and the table and the clean and sampled totals do not change; a truncated
gzip stream is BTLBF_EIO; examples/bloom_size.cpp prints the F0 the Python layer computes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import screen_cases as sc
from test_gpu_auto_query import bf  # noqa: F401  (fixture)
from test_gpu_cpp_screen import build_program

pytestmark = pytest.mark.gpu

K, S, R = 25, 1, 12
WRAP = 70


class Files:
    def __init__(self, bf, tmp):  # noqa: F811
        rng = np.random.RandomState(31)
        genome = sc.random_bases(rng, 6000)
        reads = []
        for i in range(400):
            n = [150, 151, 24, 25, 100, 0, 1200, 80][i % 8]
            o = rng.randint(0, genome.size - n + 1)
            r = genome[o:o + n].copy()
            if n and i % 11 == 0:
                r[rng.randint(0, n)] = ord("N")
            reads.append(r)
        self.reads = reads
        self.fq, self.fa = str(tmp / "reads.fq"), str(tmp / "reads.fa")
        open(self.fq, "wb").write(sc.fastq_bytes(reads))
        open(self.fa, "wb").write(sc.fasta_bytes(reads, WRAP))
        for p in (self.fq, self.fa):
            with gzip.open(p + ".gz", "wb") as z:
                z.write(open(p, "rb").read())
        self.records = self.memory(bf, reads)
        lines = [r[a:a + WRAP] for r in reads for a in range(0, r.size, WRAP)]
        self.lines = self.memory(bf, lines)

    @staticmethod
    def memory(bf, seqs):  # noqa: F811
        """(table, totals) of the sequences added from host memory"""
        c = bf.KmerCardinality(K, S, R)
        starts = np.concatenate([[0], np.cumsum([s.size for s in seqs])]).astype(np.uint64)
        c.addSeqs(np.concatenate(seqs), starts=starts)
        out = c.table(), c.totals()
        c.close()
        return out


@pytest.fixture(scope="module")
def files(bf, tmp_path_factory):  # noqa: F811
    return Files(bf, tmp_path_factory.mktemp("cardfiles"))


def from_file(bf, path, **kw):  # noqa: F811
    c = bf.KmerCardinality(K, S, R)
    st = c.addFile(path, **kw)
    out = c.table(), c.totals(), st
    c.close()
    return out


def same(note, got, want, windows_too=True):
    (t, n, _), (wt, wn) = got, want
    assert (t == wt).all(), "%s: %d counters differ" % (note, int((t != wt).sum()))
    assert n[1:] == wn[1:] and (not windows_too or n[0] == wn[0]), "%s: totals %s, expected %s" % (note, n, wn)


def test_the_input_is_worth_testing(files):
    t, n = files.records
    assert n[0] > n[1] > n[2] > 1000 and (t > 1).sum() > 100  # windows with an N; sampling; k-mers seen more than once
    assert files.lines[1][1] < n[1]  # a line of 70 bases has fewer windows than its record


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_fastq_equals_the_records_from_memory(bf, files, suffix):  # noqa: F811
    got = from_file(bf, files.fq + suffix)
    same("fastq" + suffix, got, files.records)
    st = got[2]
    assert st["n_records"] == 400 and st["n_windows"] == files.records[1][1] and st["n_hits"] == files.records[1][2]
    assert st["n_bases"] == sum(r.size for r in files.reads) and st["n_batches"] == 1


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_wrapped_fasta_as_records_and_line_by_line(bf, files, suffix):  # noqa: F811
    same("fasta records" + suffix, from_file(bf, files.fa + suffix), files.records)
    same("fasta lines" + suffix, from_file(bf, files.fa + suffix, per_line=True), files.lines)


@pytest.mark.parametrize("how", ["argument", "environment"])
def test_small_batches_rotate_the_slots_and_cut_records_without_changing_the_sketch(bf, files, how, monkeypatch):  # noqa: F811
    """batches of 700 bases: the records of 1 200 bases are cut, every other record sooner or later falls across a
    batch end, and the two device slots take turns some eighty times"""
    if how == "environment":
        monkeypatch.setenv("BTLBF_FASTX_DEV_BYTES", "700")
    kw = {"batch_bytes": 700} if how == "argument" else {}
    for path, want in ((files.fq, files.records), (files.fa + ".gz", files.records)):
        got = from_file(bf, path, **kw)
        # (a cut record is two sequences to the parser, whose overlap holds no window of its own: the windows inside
        # sequences are the same)
        same("%s in batches of 700" % os.path.basename(path), got, want)
        st = got[2]
        assert st["n_batches"] > 50 and st["n_records"] == 400
        assert st["n_bases"] > sum(r.size for r in files.reads)  # the overlaps of the cut records


def test_calls_accumulate_across_files(bf, files):  # noqa: F811
    c = bf.KmerCardinality(K, S, R)
    c.addFile(files.fq)
    st = c.addFile(files.fa + ".gz", batch_bytes=2000)
    t, n = c.table(), c.totals()
    wt, wn = files.records
    assert (t == 2 * wt).all() and n == tuple(2 * x for x in wn)
    assert st["n_windows"] == wn[1] and st["n_hits"] == wn[2]  # of the second call alone
    c.close()


def test_truncated_gzip_is_eio(bf, files, tmp_path):  # noqa: F811
    data = open(files.fq + ".gz", "rb").read()
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(data[: len(data) // 2])
    c = bf.KmerCardinality(K, S, R)
    with pytest.raises(bf._lib.BtlbfError) as e:
        c.addFile(str(cut))
    assert e.value.code == bf._lib.EIO
    c.clear()  # the sketch is usable afterwards
    c.addFile(files.fq)
    assert (c.table() == files.records[0]).all()
    c.close()


def test_example_prints_the_python_estimate(bf, files, tmp_path):  # noqa: F811
    exe = build_program(tmp_path, os.path.join("examples", "bloom_size.cpp"))
    r = subprocess.run([exe, "-k", str(K), "-s", str(S), "-r", str(R), "-p", "0.01", "-g", "4", "-t", "2", files.fq + ".gz",
                        files.fa], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = dict(ln.split("\t")[:2] for ln in r.stdout.splitlines())
    c = bf.KmerCardinality(K, S, R)
    c.addFile(files.fq + ".gz")
    c.addFile(files.fa)
    e = c.estimate(16)
    c.close()
    assert float(out["F0"]) == e.distinct and float(out["f1"]) == e.singletons and float(out["f2"]) == e.spectrum[1]
    assert int(out["records"]) == 800 and int(out["kmers"]) == e.clean_windows and int(out["sampled"]) == e.sampled
    assert abs(float(out["occupancy"]) - e.occupancy) < 1e-6
    v = int(-float(int(e.distinct)) * 4.0 / np.log(1.0 - 0.01 ** (1.0 / 4.0)))
    assert int(out["bits"]) == v + (64 - v % 64)
    assert float(out["F0_at_least_2"]) == max(e.at_least(2), 0.0)
    v2 = int(-float(int(max(e.at_least(2), 0.0))) * 4.0 / np.log(1.0 - 0.01 ** (1.0 / 4.0)))
    assert abs(int(out["bits_at_least_2"]) - (v2 + (64 - v2 % 64))) <= 64  # (libm's pow and log against numpy's)
    r = subprocess.run([exe, "-k", "25"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
