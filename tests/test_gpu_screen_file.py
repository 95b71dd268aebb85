"""The read screen over FASTA / FASTQ files (btlbf_screen_fastx_* through screenFile): rows are records in file order,
every row equals the in-memory call on the same reads, first_row is contiguous, the summary equals the numpy tally, the
statistics are filled, and parser errors come back unchanged after the batches that were complete.

About 3000 reads of mixed lengths -- empty ones, shorter than k, around 150, a few of several thousand bases -- a third
of them cut out of sequences two small filters hold; as FASTQ and as FASTA (wrapped lines), plain and gzipped; a
batch_bytes small enough for more than five batches, so that both device slots and both pinned result sets rotate."""
import gzip

import numpy as np
import pytest

import screen_cases as sc
from screen_model import tally_model, verdict_model
from test_gpu_auto_query import bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

K, H = 31, 4
SIZES = (1 << 18, 100000)
BATCH = 40000


class Files:
    def __init__(self, bf, tmp):  # noqa: F811
        rng = np.random.RandomState(55)
        genome = [sc.random_bases(rng, 20000) for _ in range(2)]
        lens = rng.choice([0, 1, 30, 31, 32, 100, 149, 150, 151, 250], 3000).tolist()
        for i in (17, 900, 2100, 2999):
            lens[i] = 4000 + i
        lens[0] = lens[1500] = 0
        reads = []
        for i, n in enumerate(lens):
            if i % 3 == 0 and n:
                o = rng.randint(0, 20000 - n)
                reads.append(genome[(i // 3) % 2][o:o + n].copy())
            else:
                reads.append(sc.random_bases(rng, n))
        reads[40][10] = ord("N")
        self.reads = reads
        self.filters = [bf.BloomFilter(b, H, K) for b in SIZES]
        for f, g in zip(self.filters, genome):
            f.insertSeqs(g)
        self.fq, self.fa = str(tmp / "reads.fq"), str(tmp / "reads.fa")
        open(self.fq, "wb").write(sc.fastq_bytes(reads))
        open(self.fa, "wb").write(sc.fasta_bytes(reads))
        for p in (self.fq, self.fa):
            with gzip.open(p + ".gz", "wb") as z:
                z.write(open(p, "rb").read())
        self.bf = bf

    def memory(self, reads, **kw):
        """the in-memory call over these reads (host buffers)"""
        buf = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
        starts = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
        return self.bf.screenSeqs(self.filters, buf, starts=starts, **kw)


@pytest.fixture(scope="module")
def files(bf, tmp_path_factory):  # noqa: F811
    return Files(bf, tmp_path_factory.mktemp("screenfile"))


def collect(it):
    firsts, parts = [], []
    for first, hits, valid, pb in it:
        firsts.append(first)
        parts.append((hits, valid, pb))
    rows = [np.concatenate([p[i] for p in parts]) for i in range(3)] if parts else None
    return firsts, [len(p[1]) for p in parts], rows


@pytest.mark.parametrize("name", ["fq", "fq.gz", "fa", "fa.gz"])
def test_rows_equal_the_in_memory_call(bf, files, name):  # noqa: F811
    path = (files.fq if name.startswith("fq") else files.fa) + (".gz" if name.endswith(".gz") else "")
    # a FASTA record without sequence lines is no row; a FASTQ record with an empty sequence line is one
    reads = files.reads if name.startswith("fq") else [r for r in files.reads if r.size]
    kw = dict(min_fraction=0.5, min_hits=3)
    exp = files.memory(reads, **kw)
    assert (exp[2] != 0).sum() > 300 and (exp[2] == 0).sum() > 300 and (exp[1] == 0).sum() > 500
    it = bf.screenFile(files.filters, path, batch_bytes=BATCH, **kw)
    firsts, sizes, rows = collect(it)
    assert len(sizes) >= 6 and firsts == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert sum(sizes) == len(reads)
    for got, want, what in zip(rows, exp, ("hits", "valid", "pass_bits")):
        assert got.shape == want.shape and (got == want).all(), (name, what, np.argwhere(got != want)[:3])
    tally = it.tally()
    assert [x.tolist() for x in tally] == [x.tolist() for x in tally_model(*exp)]
    assert next(iter(it), None) is None  # the end stays the end
    it.close()


@pytest.mark.parametrize("name", ["fq", "fa.gz"])
def test_summary_only(bf, files, name):  # noqa: F811
    path = files.fq if name == "fq" else files.fa + ".gz"
    reads = files.reads if name == "fq" else [r for r in files.reads if r.size]
    hits, valid, _ = files.memory(reads)
    pb = verdict_model(hits, valid, 0.15, 2)
    passed, best, totals, st = bf.screenFile(files.filters, path, min_fraction=0.15, min_hits=2, batch_bytes=BATCH,
                                             summary_only=True)
    assert [x.tolist() for x in (passed, best, totals)] == [x.tolist() for x in tally_model(hits, valid, pb)]
    assert totals[0] == len(reads) and passed.sum() > 0
    n_bases = sum(r.size for r in reads)
    assert st["n_bases"] == n_bases and st["n_batches"] >= 6 and st["n_batches"] <= n_bases // (BATCH // 2) + 2
    assert st["n_windows"] == int(valid.astype(np.int64).sum()) and st["n_hits"] == 0
    assert st["n_records"] == len(files.reads) if name == "fq" else st["n_records"] >= len(reads)
    assert st["seconds_total"] > 0 and 0 <= st["seconds_parse"] <= st["seconds_total"]


def test_a_batch_without_a_base(bf, files, tmp_path):  # noqa: F811
    """records with empty sequence lines only: rows of zeros"""
    p = tmp_path / "empty.fq"
    p.write_bytes(b"@a\n\n+\n\n@b\n\n+\n\n@c\n\n+\n\n")
    firsts, sizes, rows = collect(bf.screenFile(files.filters, str(p)))
    assert firsts == [0] and sizes == [3]
    assert not rows[0].any() and not rows[1].any() and not rows[2].any() and rows[0].shape == (3, 2)


def test_truncated_gzip_is_eio_after_the_complete_batches(bf, files, tmp_path):  # noqa: F811
    from btl_bloomfilter_amd import _lib

    data = open(files.fq + ".gz", "rb").read()
    cut = tmp_path / "cut.fq.gz"
    cut.write_bytes(data[: len(data) * 2 // 3])
    it = bf.screenFile(files.filters, str(cut), batch_bytes=BATCH)
    firsts, parts = [], []
    with pytest.raises(_lib.BtlbfError) as e:
        for first, hits, valid, pb in it:
            firsts.append(first)
            parts.append((hits, valid, pb))
    assert e.value.code == _lib.EIO, str(e.value)
    n = sum(len(p[1]) for p in parts)
    assert len(parts) >= 2 and 0 < n < len(files.reads)
    assert firsts == np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])[:-1]]).tolist()
    exp = files.memory(files.reads[:n])
    for i in range(3):
        assert (np.concatenate([p[i] for p in parts]) == exp[i]).all()
    with pytest.raises(_lib.BtlbfError) as e2:  # the error stays the answer
        next(it)
    assert e2.value.code == _lib.EIO
    passed, best, totals = it.tally()  # ... and the rows delivered stay counted
    assert totals[0] == n
    it.close()
    tot = bf.screenFile(files.filters, files.fq + ".gz", batch_bytes=BATCH, summary_only=True)[2]
    assert tot[0] == len(files.reads)
    with pytest.raises(_lib.BtlbfError) as e3:
        bf.screenFile(files.filters, str(cut), batch_bytes=BATCH, summary_only=True)
    assert e3.value.code == _lib.EIO


def test_a_record_longer_than_a_batch_is_einval(bf, files):  # noqa: F811
    """read 17 (the 18th record) has 4017 bases; with batches of 3000 the parser closes the batch that was open -- reads
    0..16, 1400-odd bases -- delivers it, and the next call names record 18"""
    from btl_bloomfilter_amd import _lib

    assert sum(r.size for r in files.reads[:17]) < 3000 and files.reads[17].size == 4017
    it = bf.screenFile(files.filters, files.fq, batch_bytes=3000)
    got = []
    with pytest.raises(_lib.BtlbfError) as e:
        for first, hits, valid, pb in it:
            assert first == sum(len(g[1]) for g in got)
            got.append((hits, valid, pb))
    assert e.value.code == _lib.EINVAL
    assert "record 18 is longer than a batch of 3000 bytes" in str(e.value), str(e.value)
    rows = sum(len(g[1]) for g in got)
    assert rows == 17, rows
    exp = files.memory(files.reads[:17])
    for i in range(3):
        assert (np.concatenate([g[i] for g in got]) == exp[i]).all()
    with pytest.raises(_lib.BtlbfError) as e2:  # the error stays the answer, with its message
        next(it)
    assert e2.value.code == _lib.EINVAL and "record 18" in str(e2.value)
    it.close()
