"""A miBF built from FASTA / FASTQ files (btlbf_mibf_build_fastx, MIBloomFilter.buildFromFiles) against the in-memory
stage calls over S, the files' sequences in order with their ids -- the contracts E1-E5 of include/btlbf.h:

  E1  the stage-1 body          == insertSeqs of S into an empty filter           byte for byte
  E2  data, counts after pass 2 == ONE insertIDs call over S
  E3  saturation "serial"       == ONE serial insertSaturation call over S
  E4  saturation "parallel"     == one parallel insertSaturation call per parser batch, in order (the batches read with
                                   the public parser, same flags and batch_bytes); the report sums their counts4
  E5  bits = 0                  == optimal_size(entries, h, occupancy), entries counted by pass 0 when not given

and, once per world, against tests/mibf_model.py (insert_ids, saturate_serial) over hash rows from btlbf_hash_seqs.

The sequences are the insert sequences of make_case("C5", 2) and make_case("nt3", 4) of the reference pins (40 and 17
sequences of 350 bases that share k-mers: there is saturation), with bits = optimal_size of that module so that the pins'
conditions carry over, and six more records: shorter than k, exactly k, only N, an N run in the middle, lowercase and
(FASTQ) an empty sequence line.  Three files: FASTA wrapped at 60 columns -- with a record without sequence lines, which
is no sequence --, the same kind gzip-compressed, and FASTQ.  Batches: batch_bytes equal to the longest record (every
record a batch of its own, so both device slots rotate), about three records, and the default."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import mibf_model as mm
import update_order_model as uo
from poison import POISONS, check_guards, poisoned_outputs
from test_gpu_mibf import _degenerate
from test_gpu_mibf_classify import bf  # noqa: F401  (fixture)
from test_gpu_mibf_classify_file import fastq
from test_mibf_classify_vs_ref import CFGS, K, make_case, optimal_size

pytestmark = pytest.mark.gpu
WORLDS = [("C5", 2), ("nt3", 4)]
LONGEST = 350


def fasta(path, records, gz=False, width=60):
    """records: (name, sequence bytes, or None for a record without sequence lines)"""
    text = b""
    for name, s in records:
        text += b">" + name + b" comment\n"
        if s is not None:
            text += b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width))
    with (gzip.open if gz else open)(str(path), "wb") as f:
        f.write(text)
    return str(path)


class World:
    """the three files of a configuration, S, and what the in-memory calls make of S"""

    def __init__(self, bf, cfg, id_bytes, tmp):  # noqa: F811
        self.bf, self.cfg, self.id_bytes = bf, cfg, id_bytes
        self.seeds, self.h = CFGS[cfg]
        g, _, entries, self.occ, self.reads, _, _ = make_case(cfg, id_bytes)
        self.bits = optimal_size(entries, self.h, self.occ)
        n1, n2 = len(g) // 3, 2 * len(g) // 3
        short, exact, only_n = g[0][:K - 1], g[1][:K], b"N" * 100
        n_run, lower = g[2][:100] + b"N" * 5 + g[2][105:200], g[3][:120].lower()
        parts = [g[:2] + [short] + g[2:n1 - 1] + [only_n] + g[n1 - 1:n1],
                 [exact] + g[n1:n2 - 2] + [n_run, lower] + g[n2 - 2:n2],
                 g[n2:n2 + 3] + [b""] + g[n2 + 3:]]
        rec = [[(b"s%d" % i, s) for i, s in enumerate(p)] for p in parts]
        rec[0].insert(4, (b"nothing", None))  # a FASTA record without sequence lines: not a sequence
        self.paths = [fasta(tmp / (cfg + "_a.fa"), rec[0]), fasta(tmp / (cfg + "_b.fa.gz"), rec[1], gz=True),
                      fastq(tmp / (cfg + "_c.fq"), parts[2])]
        self.per_file = [len(p) for p in parts]
        self.S = [s for p in parts for s in p]
        assert max(len(s) for s in self.S) == LONGEST and sum(len(s) == 0 for s in self.S) == 1
        self.buf = np.frombuffer(b"".join(self.S), np.uint8)
        self.starts = np.concatenate([[0], np.cumsum([len(s) for s in self.S])]).astype(np.uint64)
        self.file_of = np.repeat(np.arange(3), self.per_file)
        self.mem = {}

    def ids(self, mode, first):
        return (first + (np.arange(len(self.S)) if mode == "record" else self.file_of)).astype(np.uint32)

    def stage1(self):
        f = self.bf.BloomFilter(self.bits, self.h, K)
        if self.seeds:
            f.setSpacedSeeds(self.seeds, 1)
        f.insertSeqs(self.buf, starts=self.starts)
        return f

    def in_memory(self, mode, first):
        """-> body, (data, counts) after ONE insertIDs call, (data, counts, counts4) after ONE serial saturation more"""
        if (mode, first) not in self.mem:
            f = self.stage1()
            body = np.asarray(f.download()).tobytes()
            m = self.bf.MIBloomFilter(f, self.id_bytes)
            f.close()
            ids = self.ids(mode, first)
            m.insertIDs(self.buf, ids, starts=self.starts)
            e2 = (m.data().copy(), m.counts().copy())
            c4 = m.insertSaturation(self.buf, ids, starts=self.starts, serial=True)
            self.mem[mode, first] = (body, e2, (m.data().copy(), m.counts().copy(), c4), m)
        return self.mem[mode, first]

    def parser_batches(self, batch_bytes):
        return sum(len(list(self.bf.fastx_batches(p, K, batch_bytes=batch_bytes or 64 << 20, whole=True))) for p in self.paths)

    def build(self, **kw):
        kw.setdefault("bits", self.bits)
        return self.bf.MIBloomFilter.buildFromFiles(self.paths, K, h=self.h, seeds=self.seeds, id_bytes=self.id_bytes, **kw)


@pytest.fixture(scope="module")
def worlds(bf, tmp_path_factory):  # noqa: F811
    tmp = tmp_path_factory.mktemp("build")
    return {w: World(bf, w[0], w[1], tmp) for w in WORLDS}


@pytest.fixture(autouse=True)
def small_device_batches(monkeypatch):
    """device batches of 1 KiB wherever the variable is read (btlbf_insert_fastx); the builder's own two slots alternate
    with every parser batch, so batch_bytes = LONGEST already rotates them record by record"""
    monkeypatch.setenv("BTLBF_FASTX_DEV_BYTES", "1024")


def same(name, got, want):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), "%s: %d of %d entries differ" % (name, (g != w).sum(), g.size)


@pytest.mark.parametrize("batch_bytes", [LONGEST, 1100, 0], ids=["one_record", "three_records", "default"])
@pytest.mark.parametrize("world,mode,first", [(("C5", 2), "record", 1), (("C5", 2), "file", 7), (("nt3", 4), "record", 7),
                                              (("nt3", 4), "file", 1)], ids=["C5_u16_record_1", "C5_u16_file_7",
                                                                             "nt3_u32_record_7", "nt3_u32_file_1"])
def test_e1_e2_e3_equal_the_in_memory_calls(worlds, world, mode, first, batch_bytes):
    w = worlds[world]
    body, e2, e3, _ = w.in_memory(mode, first)
    n = len(w.S)
    # pass 2 alone, then with the serial saturation
    m, f, rep = w.build(ids=mode, first_id=first, saturation=None, batch_bytes=batch_bytes)
    assert np.asarray(f.download()).tobytes() == body  # E1
    same("data after pass 2", m.data(), e2[0])  # E2
    same("counts after pass 2", m.counts(), e2[1])
    assert rep["sat_counts4"] == [0, 0, 0, 0] and rep["batches"][3] == 0 and rep["batches"][0] == 0 and rep["entries"] == 0
    m2, f2, rep2 = w.build(ids=mode, first_id=first, saturation="serial", batch_bytes=batch_bytes)
    assert np.asarray(f2.download()).tobytes() == body
    same("data after serial saturation", m2.data(), e3[0])  # E3
    same("counts after serial saturation", m2.counts(), e3[1])
    assert rep2["sat_counts4"] == [e3[2][x] for x in ("clean", "found", "mutated", "saturated")]
    for r in (rep, rep2):
        assert r["n_records"] == n and r["records_per_file"] == w.per_file and r["longest_record"] == LONGEST
        assert r["n_ids"] == (n if mode == "record" else 3) and r["bits"] == w.bits == m.size() and r["pop"] == m.getPop()
        assert r["n_bases"] == w.buf.size
        # the parser's batches, file by file: a batch never spans two files.  A batch of just the longest record holds one
        # genome, or two of the short records
        assert r["batches"][1] == r["batches"][2] == w.parser_batches(batch_bytes)
        assert r["batches"][1] >= (n - 4 if batch_bytes == LONGEST else 3)
    assert rep2["batches"][3] == rep2["batches"][2]
    if mode == "record":
        assert e3[2]["mutated"] + e3[2]["saturated"] > 0  # the pins' sequences share k-mers


@pytest.mark.parametrize("world", WORLDS, ids=["C5_u16", "nt3_u32"])
def test_the_in_memory_result_equals_the_model(worlds, world):
    """what E1-E3 are compared with, against tests/mibf_model.py over hash rows from btlbf_hash_seqs"""
    w = worlds[world]
    body, e2, e3, _ = w.in_memory("record", 1)
    n = w.buf.size
    if w.seeds:
        hv, valid, _ = w.bf.sthash_seqs(w.buf, w.seeds, 1, K, starts=w.starts)
    else:
        hv, valid = w.bf.hash_seqs(w.buf, w.h, K, starts=w.starts)
    valid = w.bf.bits_to_bool(valid, n)
    rows = np.asarray(hv)[:n].astype(np.uint64)[valid]
    wseq = mm.window_seqs(n, w.starts)[valid]
    bits = np.zeros(w.bits, np.uint8)
    bits[(rows.ravel() % np.uint64(w.bits)).astype(np.int64)] = 1
    assert np.packbits(bits, bitorder="little").tobytes() == body
    ranks = mm.Ranks(np.frombuffer(body, np.uint8), w.bits)
    data, counts = np.zeros(ranks.pop, np.int64), np.zeros(ranks.pop, np.int64)
    ones = np.ones(len(rows), bool)
    ids = w.ids("record", 1)
    mm.insert_ids(data, counts, ranks, rows, ones, wseq, ids, w.id_bytes)
    assert data.tolist() == e2[0].tolist() and counts.tolist() == e2[1].tolist()
    c4 = mm.saturate_serial(data, counts, ranks, rows, ones, wseq, ids, w.id_bytes)
    assert data.tolist() == e3[0].tolist() and counts.tolist() == e3[1].tolist()
    assert list(c4) == [e3[2][x] for x in ("clean", "found", "mutated", "saturated")]


@pytest.mark.parametrize("batch_bytes", [800, 1400])
@pytest.mark.parametrize("world,mode", [(("C5", 2), "record"), (("nt3", 4), "record"), (("C5", 2), "file")],
                         ids=["C5_u16_record", "nt3_u32_record", "C5_u16_file"])
def test_e4_parallel_saturation_per_parser_batch(worlds, world, mode, batch_bytes):
    w = worlds[world]
    ids = w.ids(mode, 1)
    f = w.stage1()
    exp = w.bf.MIBloomFilter(f, w.id_bytes)
    f.close()
    exp.setScratchBudget(1 << 20)  # (the result does not depend on it: every batch fits)
    exp.insertIDs(w.buf, ids, starts=w.starts)
    sums, done, per_file, mutates, saturates = [0] * 4, 0, [], 0, 0
    for path in w.paths:  # the public parser: same flags, same batch_bytes
        batches = list(w.bf.fastx_batches(path, K, batch_bytes=batch_bytes, whole=True))
        per_file.append(len(batches))
        for bases, starts in batches:
            ns = len(starts) - 1
            c4 = exp.insertSaturation(np.frombuffer(bases, np.uint8), ids[done:done + ns],
                                      starts=np.asarray(starts, np.uint64), serial=False)
            done += ns
            mutates += c4["mutated"] > 0
            saturates += c4["saturated"] > 0
            sums = [a + c4[x] for a, x in zip(sums, ("clean", "found", "mutated", "saturated"))]
    assert done == len(w.S) and min(per_file) >= 2  # more than one batch per file
    m, _, rep = w.build(ids=mode, first_id=1, saturation="parallel", batch_bytes=batch_bytes, scratch_bytes=1 << 20)
    same("data", m.data(), exp.data())
    same("counts", m.counts(), exp.counts())
    print(world, mode, batch_bytes, "batches", per_file, "counts4", sums, "mutating", mutates, "saturating", saturates)
    assert rep["sat_counts4"] == sums and rep["batches"][3] == sum(per_file)
    if mode == "record":  # not vacuous: some batch mutates and some batch saturates
        assert mutates >= 1 and saturates >= 1


@pytest.mark.parametrize("world", WORLDS, ids=["C5_u16", "nt3_u32"])
def test_e5_pass_0_counts_the_entries_and_sizes_the_bit_vector(worlds, oracle, world):
    w = worlds[world]
    clean = len(uo.clean_windows(oracle, w.buf.tobytes(), K, w.h, starts=w.starts, seeds=w.seeds)[0])
    windows = sum(max(len(s) - K + 1, 0) for s in w.S)
    m, f, rep = w.build(bits=0, expected_entries=0, occupancy=w.occ, saturation=None, batch_bytes=1100)
    assert rep["entries"] == rep["clean_windows"] == clean and rep["windows"] == windows and 0 < clean < windows
    assert rep["bits"] == m.size() == f.getFilterSize() == optimal_size(clean, w.h, w.occ)
    assert rep["batches"][0] == rep["batches"][1] >= 3
    assert w.bf.MIBloomFilter.calcOptimalSize(clean, w.h, w.occ) == rep["bits"]
    # entries given: no pass 0, the same arithmetic
    m, f, rep = w.build(bits=0, expected_entries=16000, occupancy=0.5, saturation=None)
    assert rep["entries"] == 16000 and rep["batches"][0] == 0 and rep["bits"] == m.size() == optimal_size(16000, w.h, 0.5)
    # the files counted one by one
    got = [w.bf.countWindowsFile(p, K, whole=True, batch_bytes=800) for p in w.paths]
    assert sum(g["n_windows"] for g in got) == clean and sum(g["n_hits"] for g in got) == windows
    assert [g["n_batches"] >= 2 for g in got] == [True] * 3 and sum(g["n_bases"] for g in got) == w.buf.size


def window_counts(buf, k, starts=None, read_len=0):
    """(windows, clean windows) by definition: numpy, sequence by sequence"""
    ok = np.zeros(256, bool)
    ok[list(b"ACGTUacgtu") + [1, 3, 4, 5, 7]] = True  # what the hash kernels accept (csrc/seq_core.hpp base_entry)
    windows = clean = 0
    for b, e in uo.sequences(len(buf), starts, read_len):
        if e - b < k:
            continue
        bad = np.concatenate([[0], np.cumsum(~ok[buf[b:e]])])
        windows += e - b - k + 1
        clean += int((bad[k:] - bad[:-k] == 0).sum())
    return windows, clean


@pytest.mark.parametrize("poison", POISONS, ids=["ff", "a5"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["empty", "shorter_than_k", "only_n", "only_n_uniform", "zero_length_between",
                                  "read_len_k"])
def test_count_windows_on_degenerate_buffers(bf, monkeypatch, name, device, poison):  # noqa: F811
    import torch

    buf, starts, L = _degenerate(name, np.random.RandomState(31))
    exp = window_counts(buf, K, starts, L)
    assert exp[1] == (0 if name != "zero_length_between" and name != "read_len_k" else exp[0]) and (exp[0] > 0) == (
        name in ("only_n", "only_n_uniform", "zero_length_between", "read_len_k"))
    poisoned_outputs(monkeypatch, poison)
    if device:
        buf = torch.from_numpy(buf).cuda()
        starts = None if starts is None else torch.from_numpy(starts.astype(np.int64)).cuda()
    assert bf.countWindows(buf, K, starts=starts, read_len=L) == exp
    check_guards()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["ragged", "uniform", "none"])
@pytest.mark.parametrize("k", [1, 31, 200])
def test_count_windows_across_chunks_and_blocks(bf, layout, k, device):  # noqa: F811
    """100 003 bytes: thirteen chunks of 8192 bytes, four blocks, an odd tail; runs of refused bytes, lowercase, U, the
    raw codes; sequences of 0 .. 700 bytes, among them runs of more than 64 empty ones in a row.  The clean count also
    equals the valid windows of the library's own hash kernel (the predicate of seq_core.hpp)"""
    import torch

    rng = np.random.RandomState(k)
    n = 100003 if layout != "uniform" else 330 * 303
    buf = np.frombuffer(b"ACGTacgtU", np.uint8)[rng.randint(0, 9, n)].copy()
    buf[rng.randint(0, n, n // 300)] = ord("N")
    buf[rng.randint(0, n, 40)] = np.array([1, 3, 4, 5, 7, 0, 2, 6], np.uint8)[rng.randint(0, 8, 40)]
    for at in rng.randint(0, n - 500, 10):
        buf[at:at + rng.randint(1, 400)] = ord("-")
    starts, L = None, 0
    if layout == "ragged":
        lens = rng.randint(0, 701, 600)
        lens[100:180] = 0
        lens[300:400] = 0
        cuts = np.cumsum(lens)
        cuts = cuts[cuts < n]
        starts = np.concatenate([[0], cuts, [n] * 70]).astype(np.uint64)  # ... and empty ones at the very end
    elif layout == "uniform":
        L = 303
    exp = window_counts(buf, k, starts, L)
    assert 0 < exp[1] < exp[0]
    if k == 31:
        _, valid = bf.hash_seqs(buf, 1, k, starts=starts, read_len=L)
        assert int(bf.bits_to_bool(valid, n).sum()) == exp[1]
    if device:
        buf = torch.from_numpy(buf).cuda()
        starts = None if starts is None else torch.from_numpy(starts.astype(np.int64)).cuda()
    assert bf.countWindows(buf, k, starts=starts, read_len=L) == exp


def test_round_trip_store_load_classify(worlds, tmp_path):
    """the two files the build leaves, loaded again, classify the pins' reads as a miBF built in memory does"""
    w = worlds["C5", 2]
    bf_ = w.bf
    _, _, _, mem = w.in_memory("record", 1)
    m, f, rep = w.build(ids="record", first_id=1, saturation="serial", batch_bytes=1100)
    f.storeFilter(str(tmp_path / "s.bf"))
    m.store(str(tmp_path / "s.mibf"))
    f2 = bf_.BloomFilter(path=str(tmp_path / "s.bf"))
    m2 = bf_.MIBloomFilter.load(str(tmp_path / "s.mibf"), f2, w.id_bytes)
    n_ids = 1 + rep["n_ids"] + 1
    reads = fastq(tmp_path / "reads.fq", [np.frombuffer(s, np.uint8) for s in w.reads])
    rows = []
    for mi in (m2, mem):
        prob, sat = mi.calcFrameProbs(n_ids, 1)
        minc = [1] * n_ids
        got = list(mi.classifyFile(reads, prob, minc, max_miss=1, extra_frame_limit=2, max_results=3, batch_bytes=400))
        rows.append((sat, prob.tolist(), [(first, h.tobytes(), n.tolist(), s.tolist(), e.tolist()) for first, h, n, s, e in got]))
    assert rows[0] == rows[1] and sum(len(r[2]) for r in rows[0][2]) == len(w.reads)
    assert sum(int((np.asarray(r[2]) >= 1).sum()) for r in rows[0][2]) * 3 >= len(w.reads)  # a third with a result


def raw_build(w, paths, **kw):
    """the C call with both handles and the report poisoned -> (rc, message, miBF handle, stage-1 handle)"""
    L = w.bf._lib.load()
    enc = [p.encode() for p in paths]
    parr = (C.c_char_p * len(enc))(*enc)
    sarr = (C.c_char_p * len(w.seeds))(*[s.encode() for s in w.seeds]) if w.seeds else None
    p = dict(kmer_size=K, hash_num=w.h, seeds=sarr, n_seeds=len(w.seeds or ()), id_bytes=w.id_bytes, bits=w.bits,
             expected_entries=0, occupancy=w.occ, id_mode=1, first_id=1, saturation=1, fastx_flags=0, batch_bytes=0,
             scratch_bytes=0, device=0)
    p.update(kw)
    par = w.bf._lib.MibfBuildParams(**p)
    rep = w.bf._lib.MibfBuildReport()
    C.memset(C.byref(rep), 0xA5, C.sizeof(rep))
    hm, hf = C.c_void_p(0x5a5a5a5a), C.c_void_p(0xa5a5a5a5)
    rc = L.btlbf_mibf_build_fastx(C.byref(hm), C.byref(hf), parr, len(enc), C.byref(par), C.byref(rep), None)
    return rc, L.btlbf_last_error().decode(), hm.value, hf.value


def test_refusals_leave_both_handles_null(worlds, tmp_path):
    import torch

    w = worlds["C5", 2]
    lib = w.bf._lib
    # a record longer than batch_bytes: the parser's EINVAL, naming it (the third record of the first file is the
    # first of 350 bases)
    rc, msg, hm, hf = raw_build(w, w.paths, batch_bytes=LONGEST - 1)
    assert rc == lib.EINVAL and "record 1 " in msg and not hm and not hf, msg
    # per record, the last id reaches the mask of uint16_t: known after pass 1
    rc, msg, hm, hf = raw_build(w, w.paths, first_id=0x7fff - 3)
    assert rc == lib.EINVAL and "saturation mask 32768" in msg and "%d records" % len(w.S) in msg and not hm and not hf, msg
    rc, msg, hm, hf = raw_build(w, w.paths[:1], first_id=0x8000 - w.per_file[0])  # the last id is 0x7fff: it fits
    assert rc == 0 and hm and hf, msg
    L = lib.load()
    L.btlbf_mibf_destroy(C.c_void_p(hm))
    L.btlbf_destroy(C.c_void_p(hf))
    # the longest record beyond a tiny scratch budget: 350 bytes need 40 * h bytes each to be inserted
    rc, msg, hm, hf = raw_build(w, w.paths, scratch_bytes=1000)
    assert rc == lib.ENOMEM and "%d bytes would do" % (LONGEST * 40 * w.h) in msg and not hm and not hf, msg
    rc, msg, hm, hf = raw_build(w, w.paths, scratch_bytes=LONGEST * 40 * w.h - 1, saturation=0)
    assert rc == lib.ENOMEM and "insert" in msg and not hm and not hf, msg
    # an unreadable LAST path: EIO at entry, naming it, with no device memory taken
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    rc, msg, hm, hf = raw_build(w, w.paths + [str(tmp_path / "missing.fa")])
    assert rc == lib.EIO and "missing.fa" in msg and not hm and not hf, msg
    assert torch.cuda.mem_get_info()[0] >= free
    # and the miBF of a good call after all that is the in-memory one
    m, _, _ = w.build(ids="record", first_id=1, saturation="serial", batch_bytes=1100)
    same("data", m.data(), w.in_memory("record", 1)[2][0])
