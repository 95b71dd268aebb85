"""Counting filters with 16-, 32- and 64-bit counters on the GPU (BTLBF_COUNTING16 / 32 / 64: the direct path of
csrc/wide_counter_kernels.hip) against tests/wide_counter_model.py and the reference's pinned output
(tests/golden/wide_counter_vs_ref.json, tests/golden/wcbf_*.bf; tests/test_wide_counter_vs_ref.py pins the model to the
reference).  The shapes are the model's seeded cases: the 8-byte filter on which every k-mer collides, 1000 bytes (no
power of two: `% counters` differs from `% bytes`), 4096 bytes, the reference's unit-test shape; bodies prefilled from
{0, 1, 0xff, 0x100, MAX-2, MAX-1, MAX}.  Every test runs from host and from device memory; sequence buffers and hash-row
batches come below and above the sizes at which the host code goes through the pinned mailbox.  Contention comes from
the inputs of one call; nothing is run in a loop."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, load_golden

import poison
import update_order_model as uo
import wide_counter_model as wm

pytestmark = pytest.mark.gpu
WIDTHS = (16, 32, 64)
SPACES = ("host", "device")


@pytest.fixture(scope="module")
def eng():
    from btl_bloomfilter_amd import engine

    return engine


@pytest.fixture(scope="module")
def pins():
    return load_golden("wide_counter_vs_ref.json")


def put(x, mem, dtype=np.uint8):
    """a numpy array in the memory space `mem` (device: a torch tensor of torch's same-width signed type)"""
    a = np.ascontiguousarray(x, dtype)
    if mem == "host":
        return a
    import torch

    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def ragged(reads, mem):
    buf = np.frombuffer(b"".join(reads), np.uint8)
    starts = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    return put(buf, mem), put(starts, mem, np.uint64)


def rows_of(oracle, reads, h, k):
    """(byte offsets of the clean windows in the concatenated buffer, their hash rows)"""
    return uo.clean_windows(oracle, b"".join(reads), k, h, starts=np.cumsum([0] + [len(s) for s in reads]))


def new_filter(eng, bits, shape, thr=None, body=True):
    nbytes, h, k, t, reads, before = wm.make_case(shape, bits)
    f = eng.CountingBloomFilter(nbytes, h, k, t if thr is None else thr, counter_bits=bits)
    assert f.counterBytes() == bits // 8 and f.size() * (bits // 8) == f.sizeInBytes() == wm.round_bytes(nbytes)
    if body:
        f.upload(np.frombuffer(before, np.uint8))
    return f, (nbytes, h, k, t, reads, before)


def increment_all_exact(before, pos, mx):
    """saturating +1 per probe, order-free -> uint64 array"""
    add = np.bincount(np.asarray(pos, np.int64).ravel(), minlength=before.size)
    return np.array([min(int(b) + int(a), mx) for b, a in zip(before, add)], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# serial and exact paths, files
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("shape,bits,op", wm.CASES, ids=[wm.case_key(*c) for c in wm.CASES])
def test_serial_and_exact_paths_equal_model_and_reference(eng, oracle, pins, tmp_path, shape, bits, op, mem):
    f, (nbytes, h, k, thr, reads, before) = new_filter(eng, bits, shape)
    model, out, rows = wm.run_model(oracle, shape, bits, op)
    pin = pins[wm.case_key(shape, bits, op)]
    seq, starts = ragged(reads, mem)
    if op == "check":
        got = f.insertAndCheck(put(rows, mem, np.uint64), serial=True)
        assert host(got).tolist() == out
    else:
        f.insertSeqs(seq, starts=starts, increment_all=op == "all", serial=True)
    body = f.download().tobytes()
    assert body == model.body() and wm.sha(body) == pin["body_sha"]
    assert (f.counters() == model.counters()).all() and f.counters().dtype == wm.DTYPES[bits]
    b = np.frombuffer(before, wm.DTYPES[bits])
    assert (f.counters()[b == wm.max_of(bits)] == wm.max_of(bits)).all()  # a saturated counter is untouched
    if op == "all":  # ... and exact in parallel order too
        g, _ = new_filter(eng, bits, shape)
        g.insertSeqs(seq, starts=starts, increment_all=True, serial=False)
        assert g.download().tobytes() == body
        assert g.compare(f) == (0, 0, 0)
        g.close()
    # the stored file is the reference's, byte for byte
    path = tmp_path / "f.bf"
    f.storeFilter(path)
    data = path.read_bytes()
    assert wm.sha(data) == pin["file_sha"] and data == model.file_bytes()
    assert [f.popCount(), f.filtered_popcount()] == pin["pop"]
    mins = f.minCount(put(rows, mem, np.uint64))
    assert host(mins).dtype.itemsize == bits // 8
    assert host(mins).view(wm.DTYPES[bits]).tolist() == [model.min_count(r) for r in rows]
    f.close()


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("shape", ["c8", "c1000"])
@pytest.mark.parametrize("op", ["min", "all"])
def test_pinned_reference_files_load(eng, pins, tmp_path, shape, bits, op):
    path = os.path.join(GOLDEN, wm.fixture_name(shape, bits, op))
    data = open(path, "rb").read()
    cut = data.index(b"[HeaderEnd]\n") + len(b"[HeaderEnd]\n")
    nbytes, h, k, thr, _, _ = wm.make_case(shape, bits)
    f = eng.CountingBloomFilter(path=path, countThreshold=thr, counter_bits=bits)
    assert f.download().tobytes() == data[cut:] and wm.sha(data[cut:]) == pins[wm.case_key(shape, bits, op)]["body_sha"]
    assert (f.getHashNum(), f.getKmerSize(), f.sizeInBytes(), f.size()) == (h, k, len(data) - cut, (len(data) - cut) * 8 // bits)
    assert f.header() == data[:cut]
    out = tmp_path / "again.bf"
    f.storeFilter(out)
    assert out.read_bytes() == data
    # create_from_header + upload gives the same
    hnd = C.c_void_p()
    L = f._L
    assert L.btlbf_create_from_header(C.byref(hnd), wm.KINDS[bits], data[:cut], cut, thr, 0) == 0, L.btlbf_last_error()
    g = eng.CountingBloomFilter.__new__(eng.CountingBloomFilter)
    eng._Filter.__init__(g, hnd)
    g.counter_bits, g.dtype = bits, wm.DTYPES[bits]
    assert g.popCount() == 0
    g.upload(np.frombuffer(data[cut:], np.uint8))
    assert g.compare(f) == (0, 0, 0) and g.digest() == f.digest() == eng.body_digest(data[cut:])
    # loaded as another width the sizes do not fit: EFORMAT naming both numbers; as 8-bit counters: today's error
    for other in (8, 16, 32, 64):
        if other == bits:
            continue
        assert L.btlbf_load(C.byref(hnd), wm.KINDS[other], path.encode(), thr, 0) == 4
        msg = L.btlbf_last_error().decode()
        if other == 8:
            assert "only 8-bit counters are supported" in msg
        else:
            assert str(f.size()) in msg and str(f.sizeInBytes()) in msg
    # BitsPerCounter is echoed, not trusted
    odd = tmp_path / "bpc.bf"
    odd.write_bytes(data.replace(b"BitsPerCounter = 8", b"BitsPerCounter = %d" % bits))
    e = eng.CountingBloomFilter(path=odd, countThreshold=thr, counter_bits=bits)
    assert b"BitsPerCounter = %d\n" % bits in e.header() and e.compare(f) == (0, 0, 0)
    for x in (e, g, f):
        x.close()


# ---------------------------------------------------------------------------------------------------------------
# parallel order
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_parallel_increment_min_contract(eng, oracle, bits, mem):
    mx = wm.max_of(bits)
    # the contended 8-byte filter: 4 / 2 / 1 counters, every k-mer collides (16 bits: both halves of both words)
    f, (nbytes, h, k, thr, reads, before) = new_filter(eng, bits, "c8")
    _, rows = rows_of(oracle, reads, h, k)
    pos = uo.positions(rows, f.size())
    b = np.frombuffer(before, wm.DTYPES[bits]).astype(np.uint64)
    seq, starts = ragged(reads, mem)
    f.insertSeqs(seq, starts=starts)
    wm.check_increment_min(b, f.counters(), increment_all_exact(b, pos, mx), pos, mx)
    f.close()
    # duplicated rows on 1000 bytes, through the hash-row calls; insertAndCheck in parallel order as well
    for check in (False, True):
        f, (nbytes, h, k, thr, reads, before) = new_filter(eng, bits, "c1000")
        _, rows = rows_of(oracle, reads, h, k)
        rows = uo.duplicated_rows(5, rows, 1, 40)
        pos = uo.positions(rows, f.size())
        b = np.frombuffer(before, wm.DTYPES[bits]).astype(np.uint64)
        upper = increment_all_exact(b, pos, mx)
        if check:
            out = f.insertAndCheck(put(rows, mem, np.uint64), serial=False)
            wm.check_counting_insert_and_check(b, f.counters(), upper, pos, host(out), thr, mx)
        else:
            f.insert(put(rows, mem, np.uint64))
            wm.check_increment_min(b, f.counters(), upper, pos, mx)
        f.close()


# ---------------------------------------------------------------------------------------------------------------
# queries: thresholds, full-width minimum counts, both host paths, the output contract
# ---------------------------------------------------------------------------------------------------------------
def query_case(oracle, bits, n_copies):
    """the reads of the 1000-byte case, as one uniform buffer of n_copies of its first read behind a ragged head is not
    possible in one layout: so either the ragged reads (n_copies = 0) or n_copies of read 0, uniform"""
    nbytes, h, k, thr, reads, before = wm.make_case("c1000", bits)
    if n_copies:
        return [reads[0]] * n_copies, len(reads[0])
    return reads, 0


@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("n_copies", [0, 1, 1100], ids=["ragged", "one_read", "72KB"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_queries_full_width(eng, oracle, bits, n_copies, mem):
    mx = wm.max_of(bits)
    nbytes, h, k, _, _, before = wm.make_case("c1000", bits)
    reads, read_len = query_case(oracle, bits, n_copies)
    buf = b"".join(reads)
    assert n_copies != 1100 or len(buf) > 65536
    model = wm.WideCBF(bits, nbytes, h, k, 0, before)
    wpos, wrows = oracle.nthash_seq(reads[0], h, k) if n_copies else rows_of(oracle, reads, h, k)
    if n_copies:
        wpos = np.concatenate([np.asarray(wpos, np.int64) + i * read_len for i in range(n_copies)])
        mins1 = [model.min_count(r) for r in wrows]
        mins = np.array(mins1 * n_copies, dtype=np.uint64)
    else:
        mins = np.array([model.min_count(r) for r in wrows], dtype=np.uint64)
    if not n_copies:
        assert (mins > 255).any() and (mins < 256).any()  # minimum counts that do not fit a byte, and some that do
    exp_min = np.zeros(len(buf), np.uint64)
    exp_min[wpos] = mins
    valid = np.zeros(len(buf), bool)
    valid[wpos] = True
    seq = put(np.frombuffer(buf, np.uint8), mem)
    starts = None if n_copies else put(np.cumsum([0] + [len(s) for s in reads]), mem, np.uint64)
    for thr in (1, 256, mx):
        if thr > 0xffffffff:
            thr = 0xffffffff  # `threshold` is unsigned; compared against the full-width minimum
        f = eng.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
        f.upload(np.frombuffer(before, np.uint8))
        hit, vb, cnt = f.containsSeqs(seq, starts=starts, read_len=read_len, want_counts=True)
        exp_hit = valid & (exp_min >= np.uint64(thr))
        poison.assert_bitmap("hit", hit, exp_hit, len(buf))
        poison.assert_bitmap("valid", vb, valid, len(buf))
        assert host(cnt).tolist() == [int(valid.sum()), int(exp_hit.sum())]
        if thr == 256:
            mn, vb2 = f.minCountSeqs(seq, starts=starts, read_len=read_len)
            poison.assert_same("min", host(mn).view(wm.DTYPES[bits]), exp_min.astype(wm.DTYPES[bits]))
            poison.assert_bitmap("valid", vb2, valid, len(buf))
            rows = np.ascontiguousarray(np.tile(wrows, (n_copies or 1, 1)) if n_copies else wrows, np.uint64)
            got = f.contains(put(rows, mem, np.uint64))
            assert (host(got) == (mins >= np.uint64(thr))).all()
        f.close()


@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_min_count_of_many_rows_beyond_the_mailbox(eng, oracle, bits, mem):
    nbytes, h, k, thr, reads, before = wm.make_case("c1000", bits)
    model = wm.WideCBF(bits, nbytes, h, k, thr, before)
    _, rows = rows_of(oracle, reads, h, k)
    big = np.ascontiguousarray(np.tile(rows, (50000 // len(rows) + 1, 1)), np.uint64)
    assert big.nbytes > (1 << 20)
    f = eng.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
    f.upload(np.frombuffer(before, np.uint8))
    got = host(f.minCount(put(big, mem, np.uint64))).view(wm.DTYPES[bits])
    exp = np.array([model.min_count(r) for r in rows] * (50000 // len(rows) + 1), dtype=np.uint64)
    assert (got == exp.astype(wm.DTYPES[bits])).all() and (exp > 255).any()
    f.close()


def test_wide_calls_on_8_bit_counters_equal_the_byte_calls(eng, oracle):
    f = eng.CountingBloomFilter(1000, 3, 25, 1)
    reads = wm.reads_of(0, 25)
    buf = np.frombuffer(b"".join(reads), np.uint8)
    starts = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
    f.upload(uo.prefilled_counters(1, 1000))
    f.insertSeqs(buf, starts=starts, increment_all=True)
    mn, _ = f.minCountSeqs(buf, starts=starts)
    _, rows = rows_of(oracle, reads, 3, 25)
    m2 = f.minCount(rows)
    lay = eng.Layout()
    lay.starts, lay.n_seqs, lay.read_len = starts.ctypes.data, len(reads), 0
    w1 = np.full(len(buf), 0xA5, np.uint8)
    assert f._L.btlbf_min_count_seqs_wide(f._h, buf.ctypes.data, len(buf), C.byref(lay), w1.ctypes.data, None, 0, None) == 0
    w2 = np.full(len(rows), 0xA5, np.uint8)
    assert f._L.btlbf_min_count_hashes_wide(f._h, rows.ctypes.data, len(rows), w2.ctypes.data, 0, None) == 0
    assert (w1 == mn).all() and (w2 == m2).all() and f.counterBytes() == 1 and mn.any()
    f.close()


@pytest.mark.parametrize("byte", poison.POISONS)
@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_output_contract_of_the_wide_minimum_calls(eng, oracle, bits, mem, byte):
    """dirty, guarded outputs: every byte is stored (zeros of unclean windows and of the tail included), none outside"""
    nbytes, h, k, thr, reads, before = wm.make_case("c1000", bits)
    model = wm.WideCBF(bits, nbytes, h, k, thr, before)
    f = eng.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
    f.upload(np.frombuffer(before, np.uint8))
    buf = b"".join(reads)
    wpos, rows = rows_of(oracle, reads, h, k)
    exp = np.zeros(len(buf), wm.DTYPES[bits])
    exp[wpos] = [model.min_count(r) for r in rows]
    valid = np.zeros(len(buf), bool)
    valid[wpos] = True
    reg = poison.Poison(byte)
    dev = None
    if mem == "device":
        import torch

        dev = torch.device("cuda", 0)
    seq, starts = ragged(reads, mem)
    lay = eng.Layout()
    lay.starts = starts.ctypes.data if mem == "host" else starts.data_ptr()
    lay.n_seqs, lay.read_len = len(reads), 0
    sp = seq.ctypes.data if mem == "host" else seq.data_ptr()
    space = 0 if mem == "host" else 1
    mn, p_mn = reg.alloc(len(buf), wm.DTYPES[bits].newbyteorder("=") if mem == "host" else np.dtype("i%d" % (bits // 8)), dev)
    vb, p_vb = reg.alloc((len(buf) + 63) // 64, np.uint64 if mem == "host" else np.int64, dev)
    assert f._L.btlbf_min_count_seqs_wide(f._h, sp, len(buf), C.byref(lay), p_mn, p_vb, space, None) == 0
    hr = put(rows, mem, np.uint64)
    hp = hr.ctypes.data if mem == "host" else hr.data_ptr()
    m2, p_m2 = reg.alloc(len(rows), wm.DTYPES[bits].newbyteorder("=") if mem == "host" else np.dtype("i%d" % (bits // 8)), dev)
    assert f._L.btlbf_min_count_hashes_wide(f._h, hp, len(rows), p_m2, space, None) == 0
    reg.check_guards()
    poison.assert_same("min_out", mn, exp)
    poison.assert_bitmap("valid_bits", vb, valid, len(buf))
    poison.assert_same("min rows", m2, exp[wpos])
    # the byte forms on a wide filter: EINVAL, nothing written
    d8, p8 = reg.alloc(len(buf), np.uint8, dev)
    assert f._L.btlbf_min_count_seqs(f._h, sp, len(buf), C.byref(lay), p8, None, space, None) == 1
    assert f._L.btlbf_min_count_hashes(f._h, hp, len(rows), p8, space, None) == 1
    assert b"_wide" in f._L.btlbf_last_error()
    assert (poison.host_bytes(d8) == byte).all()
    f.close()


# ---------------------------------------------------------------------------------------------------------------
# reductions, refusals, the other front ends
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", WIDTHS)
def test_reductions_against_numpy(eng, bits):
    rng = np.random.RandomState(bits)
    n = 4096 * 8 // bits + 8 // (bits // 8) * 3  # (not a multiple of 16 bytes: the zero padding is not counted)
    vals = np.array(wm.prefill_values(bits) + (2, 300), dtype=np.uint64)
    a = vals[rng.randint(0, len(vals), n)].astype(wm.DTYPES[bits])
    b = a.copy()
    idx = rng.permutation(n)[: n // 3]
    b[idx] = vals[rng.randint(0, len(vals), len(idx))].astype(wm.DTYPES[bits])
    for thr in (0, 1, 256, 0xffffffff):
        fa = eng.CountingBloomFilter(a.nbytes, 2, 8, thr, counter_bits=bits)
        fb = eng.CountingBloomFilter(a.nbytes, 2, 8, thr, counter_bits=bits)
        assert fa.size() == n
        fa.upload(a.view(np.uint8))
        fb.upload(b.view(np.uint8))
        assert fa.popCount() == int((a != 0).sum())
        assert fa.filtered_popcount() == int((a.astype(np.uint64) >= np.uint64(thr)).sum())
        assert fa.compare(fb) == (int((a != b).sum()), int((a > b).sum()), int((a < b).sum()))
        assert fa.digest() == eng.body_digest(a.view(np.uint8)) and fb.digest() == eng.body_digest(b.view(np.uint8))
        fa.close()
        fb.close()


def test_refusals_on_a_wide_handle(eng):
    L = eng._lib.load()
    f = eng.CountingBloomFilter(4096, 3, 25, 1, counter_bits=32)
    for mode in ("auto", "direct"):
        f.setInsertMode(mode)
        f.setQueryMode(mode)
    out4 = (C.c_uint32 * 4)()
    u64 = C.c_uint64()
    u32a, u32b = C.c_uint(), C.c_uint()
    dbl = C.c_double()
    calls = [
        lambda: L.btlbf_set_insert_mode(f._h, 2, 0), lambda: L.btlbf_set_query_mode(f._h, 2),
        lambda: L.btlbf_store_shard(f._h, b"/nonexistent/x.bf"),
        lambda: L.btlbf_positions_seqs(f._h, None, 0, None, 1, None, None, 0, None, None, None),
        lambda: L.btlbf_insert_positions(f._h, None, 0, None), lambda: L.btlbf_test_positions(f._h, None, 0, None, None),
        lambda: L.btlbf_route_plan(f._h, 1000, None, 1, C.byref(u64), C.byref(u64)),
        lambda: L.btlbf_route_windows(f._h, 1, C.byref(u32a), C.byref(u32b)),
        lambda: L.btlbf_route_seqs(f._h, None, 0, None, 0, 1, 0, 0, None, None, None, None, None, None, 0, None, None),
        lambda: L.btlbf_route_geometry(f._h, 1000, None, 1, 0, out4),
        lambda: L.btlbf_owner_scratch_bytes(f._h, 1000, None, 1, 0, C.byref(u64)),
        lambda: L.btlbf_apply_routed_bins(f._h, None, None, 1, 0, 1, 1000, None, 1, 0, None, 0, None, None),
        lambda: L.btlbf_apply_routed(f._h, None, None, 1, 1000, None, 1, 0, None, 0, None, None),
        lambda: L.btlbf_apply_spill(f._h, None, 0, 0, None, 0, None, None),
        lambda: L.btlbf_resolve_seqs(f._h, None, 0, None, None, 0, None, None),
        lambda: L.btlbf_microbench(f._h, 0, 1000, C.byref(u64), C.byref(dbl)),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert b"direct path only" in L.btlbf_last_error(), i
    hnd = C.c_void_p()
    assert L.btlbf_rank_create(C.byref(hnd), f._h) == 1 and L.btlbf_mibf_create(C.byref(hnd), f._h, 2) == 1
    f.close()


@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_spaced_seeds(eng, oracle, bits, mem):
    seeds, h2, k = ["1110111011101110111011101", "1011101110111011101110111"], 2, 25
    h = len(seeds) * h2
    nbytes, _, _, thr, reads, before = wm.make_case("c1000", bits)
    f = eng.CountingBloomFilter(nbytes, h, k, 256, counter_bits=bits)
    f.setSpacedSeeds(seeds, h2)
    f.upload(np.frombuffer(before, np.uint8))
    model = wm.WideCBF(bits, nbytes, h, k, 256, before)
    wpos, rows = uo.clean_windows(oracle, b"".join(reads), k, h, starts=np.cumsum([0] + [len(s) for s in reads]), seeds=seeds, h2=h2)
    for r in rows:
        model.increment_all(r)
    seq, starts = ragged(reads, mem)
    f.insertSeqs(seq, starts=starts, increment_all=True)
    assert f.download().tobytes() == model.body()
    n = len(b"".join(reads))
    exp = np.zeros(n, np.uint64)
    exp[wpos] = [model.min_count(r) for r in rows]
    mn, vb = f.minCountSeqs(seq, starts=starts)
    poison.assert_same("min", host(mn).view(wm.DTYPES[bits]), exp.astype(wm.DTYPES[bits]))
    hit, _, _ = f.containsSeqs(seq, starts=starts)
    valid = np.zeros(n, bool)
    valid[wpos] = True
    poison.assert_bitmap("hit", hit, valid & (exp >= 256), n)
    f.close()


@pytest.mark.parametrize("shape", ["c1000", "c4096", "c8"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_spaced_seeds_parallel_insert_and_every_modulus(eng, oracle, bits, shape):
    """the fused kernel's incrementMin with spaced seeds (the serial order goes through hash rows), on a size that is a
    power of two, one that is not, and the 8-byte filter; three seeds with one extra hash each and h2 = 1 as well"""
    mx = wm.max_of(bits)
    for seeds, h2 in ((["1110111011101110111011101", "1011101110111011101110111", "1111100000111110000011111"], 2),
                      (["1101101101101101101101101", "1011011011011011011011011"], 1)):
        k, h = 25, len(seeds) * h2
        nbytes, _, _, _, _, _ = wm.make_case(shape, bits)
        reads = wm.reads_of(1, k)
        n_ctr = wm.round_bytes(nbytes) * 8 // bits
        before = wm.prefilled_body(bits, n_ctr, 11)
        f = eng.CountingBloomFilter(nbytes, h, k, 1, counter_bits=bits)
        f.setSpacedSeeds(seeds, h2)
        f.upload(np.frombuffer(before, np.uint8))
        wpos, rows = uo.clean_windows(oracle, b"".join(reads), k, h, starts=np.cumsum([0] + [len(s) for s in reads]), seeds=seeds, h2=h2)
        pos = uo.positions(rows, f.size())
        b = np.frombuffer(before, wm.DTYPES[bits]).astype(np.uint64)
        upper = increment_all_exact(b, pos, mx)
        seq, starts = ragged(reads, "device")
        f.insertSeqs(seq, starts=starts)
        wm.check_increment_min(b, f.counters(), upper, pos, mx)
        g = eng.CountingBloomFilter(nbytes, h, k, 1, counter_bits=bits)
        g.setSpacedSeeds(seeds, h2)
        g.upload(np.frombuffer(before, np.uint8))
        g.insertSeqs(seq, starts=starts, increment_all=True)
        wm.check_increment_all(g.counters(), upper)
        mn, _ = g.minCountSeqs(seq, starts=starts)
        exp = np.zeros(len(b"".join(reads)), np.uint64)
        exp[wpos] = upper[pos].min(axis=1)
        poison.assert_same("min", host(mn).view(wm.DTYPES[bits]), exp.astype(wm.DTYPES[bits]))
        f.close()
        g.close()


@pytest.mark.parametrize("mem", SPACES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_raw_kmers(eng, oracle, bits, mem):
    k, h = 20, 3
    nbytes, _, _, _, _, before = wm.make_case("c1000", bits)
    rng = np.random.RandomState(7)
    kmers = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for _ in range(12)]
    kmers += kmers[:5] + [b"ATCGGGUCATCAACCAATAC"]
    hv, ok = oracle.kmer_hashes(b"".join(kmers), k, h)
    assert ok.all()
    model = wm.WideCBF(bits, nbytes, h, k, 257, before)
    for r in hv:
        model.increment_min(r)
    f = eng.CountingBloomFilter(nbytes, h, k, 257, counter_bits=bits)
    f.upload(np.frombuffer(before, np.uint8))
    buf = put(np.frombuffer(b"".join(kmers), np.uint8), mem)
    f.insertKmers(buf, serial=True)
    assert f.download().tobytes() == model.body()
    got = host(f.containsKmers(buf))
    assert got.tolist() == [int(model.contains(r)) for r in hv] and 0 < got.sum() < len(got)
    f.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_fasta_ingestion(eng, oracle, bits, tmp_path):
    nbytes, h, k, _, reads, before = wm.make_case("c4096", bits)
    fa = tmp_path / "r.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(reads)))
    f = eng.CountingBloomFilter(nbytes, h, k, 2, counter_bits=bits)
    st = f.insertFile(fa)
    assert st["n_records"] == len(reads)
    # (insertFile = incrementMin in parallel order: the contract, not a body)
    _, rows = rows_of(oracle, reads, h, k)
    pos = uo.positions(rows, f.size())
    zero = np.zeros(f.size(), np.uint64)
    wm.check_increment_min(zero, f.counters(), increment_all_exact(zero, pos, wm.max_of(bits)), pos, wm.max_of(bits))
    q = f.containsFile(fa)
    buf = np.frombuffer(b"".join(reads), np.uint8)
    _, _, cnt = f.containsSeqs(buf, starts=np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64), want_counts=True)
    assert [q["n_windows"], q["n_hits"]] == cnt.tolist() and cnt[0] == len(rows) and 0 < cnt[1]
    f.close()


_CHILD = """
import sys, hashlib
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import wide_counter_model as wm
from btl_bloomfilter_amd import engine
nbytes, h, k, thr, reads, before = wm.make_case("c1000", 16)
f = engine.CountingBloomFilter(nbytes, h, k, thr, counter_bits=16)
f.upload(np.frombuffer(before, np.uint8))
buf = np.frombuffer(b"".join(reads), np.uint8)
starts = np.cumsum([0] + [len(s) for s in reads]).astype(np.uint64)
f.insertSeqs(buf, starts=starts, increment_all=True)
_, _, cnt = f.containsSeqs(buf, starts=starts, want_counts=True)
print("RESULT", hashlib.sha256(f.download().tobytes()).hexdigest(), int(cnt[0]), int(cnt[1]))
"""


def test_partitioned_modes_in_the_environment_are_ignored(eng, oracle, pins):
    """the one test that starts a process: the environment is read when a filter is made"""
    env = dict(os.environ, BTLBF_INSERT_MODE="partitioned", BTLBF_QUERY_MODE="partitioned")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][0].split()
    model, _, rows = wm.run_model(oracle, "c1000", 16, "all")
    hits = sum(1 for x in rows if model.contains(x))
    assert line[1] == pins["c1000_u16_all"]["body_sha"] == hashlib.sha256(model.body()).hexdigest()
    assert [int(line[2]), int(line[3])] == [len(rows), hits]
