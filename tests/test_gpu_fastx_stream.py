"""The file path's two device slots (run_fastx in csrc/fastx.cpp) at sizes where they rotate.

insertFile / containsFile append the parser's host batches to one of two device batches, launch a full one on the compute
stream and take the other; before a slot is reused its `done` event is waited for and its counts are harvested from a
pinned mirror.  A device batch is at least 256 MiB unless BTLBF_FASTX_DEV_BYTES says otherwise, so here it is 4 KiB (D) over
host batches of 1 KiB: files of some 60 KB take 15-20 device batches and every slot is reused many times.  Everything is
integer work and compared exactly: the filter bytes with oracle.bf_insert_seq per sequence, the counts with
oracle.nthash_seq + oracle.bf_contains, the number of device batches with a replay of the slot rule over the parser's own
batches (fastx_batches, which tests/test_fastx.py checks against Python).

Not covered: the slot switch on the SEQUENCE count.  A slot holds D/16 + 4096 sequences, so it fills up on sequences
before bases only when sequences average under 16 bases at a 256 MiB slot; at a small D the constant 4096 keeps that
switch out of reach, and the constant is not a thing to change for a test."""
import gzip
import random

import numpy as np
import pytest

from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)
from test_gpu_mibf_classify_file import PARAMS, collect, fastq, files, kw  # noqa: F401  (files: fixture)

pytestmark = pytest.mark.gpu

BITS, H = 1 << 20, 3
BATCH, D = 1024, 4096


def rand_read(rng, n, clean=False):
    s = [rng.choice("ACGT") for _ in range(n)]
    if not clean:
        if rng.random() < 0.1:  # a few Ns
            for _ in range(rng.randrange(1, 3)):
                s[rng.randrange(n)] = "N"
        if rng.random() < 0.3:  # lower case, whole or in part
            a = rng.randrange(n) if rng.random() < 0.5 else 0
            s[a:] = [c.lower() for c in s[a:]]
    return "".join(s)


def make_reads(rng, k, n=600):
    reads = [rand_read(rng, rng.randrange(60, 151)) for _ in range(n)]
    reads[n // 3] = rand_read(rng, k - 1)  # two reads shorter than k
    reads[2 * n // 3] = rand_read(rng, 3)
    return reads


def write_fastq(path, reads, rng, gz=False):
    text = "".join("@r%d x\n%s\n+\n%s\n" % (i, s, "".join(rng.choice("@>+IJ#") for _ in s)) for i, s in enumerate(reads))
    with (gzip.open if gz else open)(str(path), "wb") as f:
        f.write(text.encode())
    return path


def write_fasta(path, reads, width=60):
    """multi-line FASTA -> the sequence lines (what per_line=True makes sequences of)"""
    lines, seq_lines = [], []
    for i, s in enumerate(reads):
        lines.append(">c%d" % i)
        for a in range(0, len(s), width):
            lines.append(s[a:a + width])
            seq_lines.append(s[a:a + width])
    path.write_bytes(("\n".join(lines) + "\n").encode())
    return seq_lines


class Expected:
    """the oracle's filter bytes after inserting `seqs`, and its clean-window count"""

    def __init__(self, oracle, seqs, k, bits=BITS, h=H):
        self.array = np.zeros(bits // 8, np.uint8)
        self.n_clean = 0
        for s in seqs:
            oracle.bf_insert_seq(self.array, bits, h, k, s.encode())
            self.n_clean += len(oracle.nthash_seq(s.encode(), h, k)[0])


def query_counts(oracle, array, seqs, k, bits=BITS, h=H):
    """(clean windows, windows found in `array`) of the sequences"""
    nw = nh = 0
    for s in seqs:
        _, hv = oracle.nthash_seq(s if isinstance(s, bytes) else s.encode(), h, k)
        if len(hv):
            nw += len(hv)
            nh += int(oracle.bf_contains(array, bits, h, hv).sum())
    return nw, nh


def replay_batches(host, d=D):
    """run_fastx's slot rule over the parser's host batches: a host batch that does not fit the bases or the sequences
    left in the device batch starts the next one -> the device batches, each the list of its host batches (bases, starts)"""
    out, cur, nb, ns = [], [], 0, 0
    for bases, starts in host:
        nbi, nsi = len(bases), len(starts) - 1
        if nb + nbi > d or ns + nsi > d // 16 + 4096:
            if ns:  # a device batch counts when it holds a sequence
                out.append(cur)
            cur, nb, ns = [], 0, 0
        cur.append((bases, starts))
        nb += nbi
        ns += nsi
    if ns:
        out.append(cur)
    return out


def replay(m, path, k, per_line=False, d=D):
    return replay_batches(m.fastx_batches(path, k, per_line=per_line, batch_bytes=BATCH), d)


def pieces(dev_batch):
    return [bases[a:b] for bases, starts in dev_batch for a, b in zip(starts, starts[1:])]


@pytest.fixture
def small_slots(monkeypatch):
    monkeypatch.setenv("BTLBF_FASTX_DEV_BYTES", str(D))
    monkeypatch.setenv("BTLBF_FASTX_THREADS", "1")
    monkeypatch.setenv("BTLBF_FASTX_MT_MIN_BYTES", str(1 << 40))
    return monkeypatch


@pytest.mark.parametrize("kind", ["fastq", "fasta", "fasta_lines", "fastq_gz"])
def test_rotation_one_parser(tmp_path, oracle, small_slots, kind):
    import btl_bloomfilter_amd as m

    k = 11 if kind.startswith("fasta") else 31
    rng = random.Random(101)
    reads = make_reads(rng, k)
    per_line = kind == "fasta_lines"
    if kind.startswith("fasta"):
        path = tmp_path / "reads.fa"
        lines = write_fasta(path, reads)
        seqs = lines if per_line else reads
        assert any(len(s) < k for s in seqs)
    else:
        path = write_fastq(tmp_path / ("reads.fq.gz" if kind == "fastq_gz" else "reads.fq"), reads, rng, gz=kind == "fastq_gz")
        seqs = reads
    exp = Expected(oracle, seqs, k)
    want_batches = len(replay(m, path, k, per_line))
    f = m.BloomFilter(BITS, H, k)
    st = f.insertFile(path, per_line=per_line, batch_bytes=BATCH)
    print(kind, "insert", st)
    assert np.array_equal(f.download(), exp.array)
    assert st["n_batches"] == want_batches and want_batches >= 10
    q = f.containsFile(path, per_line=per_line, batch_bytes=BATCH)
    print(kind, "contains", q, "oracle clean windows", exp.n_clean)
    assert q["n_windows"] == exp.n_clean and q["n_hits"] == exp.n_clean
    assert q["n_batches"] == want_batches
    assert np.array_equal(f.download(), exp.array)  # a query leaves the filter alone


def partial_hit_reads(rng, k, reads_a, n=450):
    """reads of A, foreign reads, and reads whose first half is the first half of a read of A, interleaved"""
    out = []
    for i in range(n):
        a = reads_a[rng.randrange(len(reads_a))]
        if i % 3 == 0:
            out.append(a)
        elif i % 3 == 1:
            out.append(rand_read(rng, rng.randrange(60, 151)))
        else:
            out.append(a[:len(a) // 2] + rand_read(rng, rng.randrange(40, 90), clean=True))
    return out


def test_partial_hits(tmp_path, oracle, small_slots):
    import btl_bloomfilter_amd as m

    k = 31
    rng = random.Random(202)
    reads_a = make_reads(rng, k)
    path_a = write_fastq(tmp_path / "a.fq", reads_a, rng)
    reads_b = partial_hit_reads(rng, k, reads_a)
    path_b = write_fastq(tmp_path / "b.fq", reads_b, rng)
    exp = Expected(oracle, reads_a, k)
    nw, nh = query_counts(oracle, exp.array, reads_b, k)
    # per device batch, from the pieces the parser cuts: they sum to the totals, and no one of them divides a total
    dev = replay(m, path_b, k)
    per_batch = [query_counts(oracle, exp.array, pieces(b), k) for b in dev]
    assert (sum(w for w, _ in per_batch), sum(h for _, h in per_batch)) == (nw, nh)
    print("oracle windows", nw, "hits", nh, "device batches", len(dev), "per batch", per_batch)
    assert 0 < nh < nw and len(dev) >= 10
    for w, h in per_batch:
        assert (w == 0 or nw % w) and (h == 0 or nh % h)
    f = m.BloomFilter(BITS, H, k)
    f.insertFile(path_a, batch_bytes=BATCH)
    assert np.array_equal(f.download(), exp.array)
    q = f.containsFile(path_b, batch_bytes=BATCH)
    print("contains", q)
    assert (q["n_windows"], q["n_hits"], q["n_batches"]) == (nw, nh, len(dev))


def test_last_device_batch_shorter_than_k(tmp_path, oracle, small_slots):
    """B ends with a read of fewer than k bases that is a host batch of its own (the read before it fills its host batch
    to the last byte) and, at the D found here, a device batch of its own: it tests nothing and inserts nothing, and the
    slot it lands in, which held a batch two batches earlier, must not report that batch's counts again"""
    import btl_bloomfilter_amd as m

    k = 31
    rng = random.Random(303)
    reads_a = make_reads(rng, k)
    path_a = write_fastq(tmp_path / "a.fq", reads_a, rng)
    reads_b = partial_hit_reads(rng, k, reads_a)
    path_b = tmp_path / "b.fq"
    # a clean read that ends exactly where its host batch ends (a batch full at a line end carries nothing over) ...
    while True:
        write_fastq(path_b, reads_b, rng)
        host = list(m.fastx_batches(path_b, k, batch_bytes=BATCH))
        n_host, fill = len(host), len(host[-1][0])
        if BATCH - fill >= 2 * k and n_host % 4 == 0:  # four host batches to a device batch of 4 KiB come out even
            break
        reads_b.append(rand_read(rng, 100))
    reads_b.append(rand_read(rng, BATCH - fill, clean=True))
    reads_b.append("ACGTACGTAC"[:k - 1])  # ... and the short read
    write_fastq(path_b, reads_b, rng)
    host = list(m.fastx_batches(path_b, k, batch_bytes=BATCH))
    assert len(host[-2][0]) == BATCH and host[-1][0] == reads_b[-1].encode() and len(host[-1][1]) == 2
    found = None
    for d in range(2 * D - 1, BATCH - 1, -1):  # the largest first: several host batches per device batch where that works
        dev = replay_batches(host, d)
        # alone in the last device batch, whose slot has been used many times before
        if len(dev[-1]) == 1 and dev[-1][0][0] == host[-1][0] and len(dev) >= 10:
            found = d
            break
    assert found is not None
    print("D", found, "device batches", len(dev), "host batches", len(host))
    small_slots.setenv("BTLBF_FASTX_DEV_BYTES", str(found))
    exp_a = Expected(oracle, reads_a, k)
    nw, nh = query_counts(oracle, exp_a.array, reads_b, k)
    assert 0 < nh < nw
    f = m.BloomFilter(BITS, H, k)
    f.insertFile(path_a, batch_bytes=BATCH)
    q = f.containsFile(path_b, batch_bytes=BATCH)
    print("contains", q, "oracle", nw, nh)
    assert (q["n_windows"], q["n_hits"], q["n_batches"]) == (nw, nh, len(dev))
    # insert mode: the array is what the reads before the short one make it
    g = m.BloomFilter(BITS, H, k)
    st = g.insertFile(path_b, batch_bytes=BATCH)
    assert st["n_batches"] == len(dev)
    assert np.array_equal(g.download(), Expected(oracle, reads_b[:-1], k).array)


@pytest.mark.parametrize("threads", [3, 5])
def test_several_parser_threads(tmp_path, oracle, small_slots, threads):
    """the order of the host batches is the threads' business: the array and the counts are not"""
    import btl_bloomfilter_amd as m

    small_slots.setenv("BTLBF_FASTX_THREADS", str(threads))
    small_slots.setenv("BTLBF_FASTX_MT_MIN_BYTES", "0")
    k = 11
    rng = random.Random(404 + threads)
    reads = make_reads(rng, k)
    fq = write_fastq(tmp_path / "reads.fq", reads, rng)
    fa = tmp_path / "reads.fa"
    lines = write_fasta(fa, reads)
    for path, per_line, seqs in ((fq, False, reads), (fa, False, reads), (fa, True, lines)):
        exp = Expected(oracle, seqs, k)
        f = m.BloomFilter(BITS, H, k)
        st = f.insertFile(path, per_line=per_line, batch_bytes=BATCH)
        print(path.name, per_line, "insert", st)
        assert np.array_equal(f.download(), exp.array)
        assert st["n_bases"] >= sum(len(s) for s in seqs)
        assert st["n_batches"] >= -(-st["n_bases"] // D) >= 10
        q = f.containsFile(path, per_line=per_line, batch_bytes=BATCH)
        print(path.name, per_line, "contains", q)
        assert q["n_windows"] == exp.n_clean and q["n_hits"] == exp.n_clean
        assert q["n_batches"] >= -(-q["n_bases"] // D)


@pytest.mark.parametrize("threads", [1, 3])
def test_counting_filter_every_window_once(tmp_path, oracle, small_slots, threads):
    """h = 1: the parallel incrementMin is exact, so the counters are the histogram of the clean windows' hashes.  Contigs
    of some 4000 bases over eighteen repeat units are cut into host batches with k-1 bases of overlap many times, and with
    three parsers their byte ranges meet inside the file: a window applied twice or not at all changes a counter"""
    import btl_bloomfilter_amd as m

    small_slots.setenv("BTLBF_FASTX_THREADS", str(threads))
    small_slots.setenv("BTLBF_FASTX_MT_MIN_BYTES", "0" if threads > 1 else str(1 << 40))
    k = 31
    rng = random.Random(505)
    units = [rand_read(rng, rng.randrange(40, 91)) for _ in range(18)]
    contigs = ["".join(rng.choice(units) for _ in range(60)) for _ in range(12)]
    assert min(len(c) for c in contigs) > 3 * BATCH
    path = tmp_path / "repeats.fa"
    write_fasta(path, contigs)
    f = m.CountingBloomFilter(1 << 16, 1, k)
    size = f.size()
    hv = np.concatenate([oracle.nthash_seq(c.encode(), 1, k)[1][:, 0] for c in contigs])
    counts = np.bincount((hv % np.uint64(size)).astype(np.int64), minlength=size)
    exp = np.minimum(counts, 255).astype(np.uint8)
    mult = counts[counts > 0]
    print("windows", hv.size, "counters in use", mult.size, "multiplicity: median", int(np.median(mult)), "max", int(mult.max()))
    assert ((mult >= 2) & (mult <= 50)).sum() > mult.size // 2 and (mult == 1).any()
    st = f.insertFile(path, batch_bytes=BATCH)
    print("insert", st)
    assert st["n_batches"] >= 10
    got = f.download()
    assert got.dtype == np.uint8 and got.size == size
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (bad[:10], got[bad[:10]], exp[bad[:10]])
    g = m.CountingBloomFilter(1 << 16, 1, k, countThreshold=2)
    assert g.size() == size
    g.insertFile(path, batch_bytes=BATCH)
    q = g.containsFile(path, batch_bytes=BATCH)
    want = int((exp[(hv % np.uint64(size)).astype(np.int64)] >= 2).sum())
    print("contains", q, "oracle", hv.size, want)
    assert 0 < want < hv.size
    assert (q["n_windows"], q["n_hits"]) == (hv.size, want)


def truncate(path, out):
    data = open(str(path), "rb").read()
    with open(str(out), "wb") as f:
        f.write(data[:len(data) // 2])
    return out


def test_read_error_in_mid_stream(tmp_path, oracle, small_slots):
    """a gzipped FASTQ cut in half: device batches have been launched when the parser meets the end of the data; both calls
    fail with EIO, and the filter goes on working"""
    import btl_bloomfilter_amd as m
    from btl_bloomfilter_amd._lib import EIO, BtlbfError

    k = 31
    rng = random.Random(606)
    reads = make_reads(rng, k)
    good = write_fastq(tmp_path / "reads.fq.gz", reads, rng, gz=True)
    cut = truncate(good, tmp_path / "cut.fq.gz")
    # the parser alone: at least three device batches' worth of host batches before the error
    n_host = 0
    with pytest.raises(BtlbfError) as e:
        for _ in m.fastx_batches(cut, k, batch_bytes=BATCH):
            n_host += 1
    assert e.value.code == EIO and n_host * BATCH >= 3 * D
    f = m.BloomFilter(BITS, H, k)
    for call in (f.insertFile, f.containsFile):
        with pytest.raises(BtlbfError) as e:
            call(cut, batch_bytes=BATCH)
        assert e.value.code == EIO and "cut.fq.gz" in str(e.value), str(e.value)
    f.clear()
    assert not f.download().any()
    exp = Expected(oracle, reads, k)
    f.insertFile(good, batch_bytes=BATCH)
    assert np.array_equal(f.download(), exp.array)
    q = f.containsFile(good, batch_bytes=BATCH)
    assert q["n_windows"] == exp.n_clean == q["n_hits"]


@pytest.mark.parametrize("damaged", ["path1", "path2"])
def test_classify_file_read_error(files, bf, tmp_path, damaged):  # noqa: F811
    """one of the two mate files is a .gz cut in half: EIO, not fewer rows and not `the two files do not pair up`; the rows
    delivered before the error are the pairs' rows"""
    c, p = files.case, PARAMS[0]
    exp = files.mem["pairs", p]
    f1 = fastq(tmp_path / "r1.fq.gz", files.m1, gz=True)
    f2 = fastq(tmp_path / "r2.fq.gz", files.m2, gz=True)
    if damaged == "path1":
        f1 = str(truncate(f1, tmp_path / "cut1.fq.gz"))
    else:
        f2 = str(truncate(f2, tmp_path / "cut2.fq.gz"))
    it = c.m.classifyFile(f1, c.prob, c.minc, path2=f2, batch_bytes=300, **kw(p))
    with pytest.raises(bf._lib.BtlbfError) as ei:
        collect(it, exp)
    assert ei.value.code == bf._lib.EIO and "pair up" not in str(ei.value) and "cut" in str(ei.value), str(ei.value)
    rows = it.tally()[2][0]
    print(damaged, "rows before the error", rows, "|", ei.value)
    assert rows < len(exp[1])
    it.close()
    with pytest.raises(bf._lib.BtlbfError) as ei:
        c.m.classifyFile(f1, c.prob, c.minc, path2=f2, batch_bytes=300, summary_only=True, **kw(p))
    assert ei.value.code == bf._lib.EIO
    # the miBF is as it was
    assert collect(c.m.classifyFile(files.f1, c.prob, c.minc, path2=files.f2, batch_bytes=300, **kw(p)), exp, 5) == len(exp[1])
