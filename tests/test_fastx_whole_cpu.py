"""BTLBF_FASTX_WHOLE, the parser mode of the file classifier (no GPU): every record is one whole sequence in exactly one
batch, in file order, whatever the batch size down to the longest record; an empty FASTQ read is an empty sequence; a
record longer than a batch is EINVAL naming the record; without the flag nothing changes."""
import gzip

import numpy as np
import pytest


def write_fastq(path, reads, crlf=False, gz=False):
    nl = b"\r\n" if crlf else b"\n"
    text = b"".join(b"@r%d" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(reads))
    with (gzip.open if gz else open)(str(path), "wb") as f:
        f.write(text)
    return str(path)


def reads_of(seed, n=60):
    rng = np.random.RandomState(seed)
    lens = [0, 1, 30, 31, 97, 150] + list(rng.randint(0, 151, n - 6))
    return [bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.randint(0, 5, L)]) for L in lens]


def parsed(path, batch_bytes, **kw):
    from btl_bloomfilter_amd import fastx_batches

    out, sizes = [], []
    for bases, starts in fastx_batches(path, 31, batch_bytes=batch_bytes, whole=True, **kw):
        assert starts[0] == 0 and starts[-1] == len(bases) and len(bases) <= max(batch_bytes, 1)
        out += [bases[a:b] for a, b in zip(starts, starts[1:])]
        sizes.append(len(starts) - 1)
    return out, sizes


@pytest.mark.parametrize("crlf,gz", [(False, False), (True, False), (False, True)])
def test_whole_records_in_order_for_every_batch_size(lib, tmp_path, crlf, gz):
    reads = reads_of(1)
    path = write_fastq(tmp_path / "a.fq", reads, crlf, gz)
    for batch in (150, 151, 200, 299, 300, 1000, 1 << 20):
        got, sizes = parsed(path, batch)
        assert got == reads, batch
        if batch < 1000:
            assert len(sizes) > 10
    assert parsed(path, 150)[1] != parsed(path, 200)[1]


def test_a_record_longer_than_a_batch_is_named(lib, tmp_path):
    from btl_bloomfilter_amd import _lib

    reads = [b"ACGT" * 10, b"ACGT" * 5, b"A" * 100, b"ACGT" * 10]
    path = write_fastq(tmp_path / "a.fq", reads)
    assert parsed(path, 100)[0] == reads
    with pytest.raises(_lib.BtlbfError) as ei:
        parsed(path, 99)
    assert ei.value.code == _lib.EINVAL and "record 3 " in str(ei.value)


def test_multi_line_fasta_records_stay_whole(lib, tmp_path):
    recs = [b"ACGTACGTAC" * 7, b"", b"TTTTGGGGCC" * 3, b"ACGTACGTAC" * 7]
    text = b"".join(b">c%d\n" % i + b"".join(s[j:j + 10] + b"\n" for j in range(0, len(s), 10)) for i, s in enumerate(recs))
    path = tmp_path / "a.fa"
    path.write_bytes(text)
    for batch in (70, 71, 100, 140, 1000):
        got, _ = parsed(str(path), batch)
        assert got == [r for r in recs if r], batch  # a FASTA record without sequence lines has no sequence


def test_without_the_flag_a_long_sequence_is_still_cut(lib, tmp_path):
    from btl_bloomfilter_amd import fastx_batches

    path = write_fastq(tmp_path / "a.fq", [b"ACGT" * 100, b""])
    got = list(fastx_batches(path, 31, batch_bytes=200))
    assert len(got) == 3 and sum(len(s) - 1 for _, s in got) == 3  # two cuts with a 30-base overlap, no empty sequence
