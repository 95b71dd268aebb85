"""The read-modify-write kernels in PARALLEL order -- the order callers get by default -- against the atomic contract
of tests/update_order_model.py: insertAndCheck on bit filters, incrementAll / incrementMin / insertAndCheck on counting
filters, through sequence buffers (pinned mailbox, staged host buffer, device tensor at odd alignments) and hash rows.

Where the input makes the result order-free (windows that share no position, though they do share 32-bit words) the
comparison with the serial oracle is bit-exact; where windows fight over positions the result must be one that SOME
interleaving of the reference's per-probe atomics produces: properties P1-P6, A1, M1-M4 (tests/test_update_order_cpu.py
shows that they accept every interleaving and reject the usual mistakes).  Every comparison is integer-exact or a stated
inequality; preconditions are asserted on oracle data before the GPU call."""
import ctypes as C

import numpy as np
import pytest

import update_order_model as m

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bf():
    # torch first, as in every production flow (bench.py, smoke(), the sharded path): its HIP runtime
    # and context are up before the library makes its first call
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    import btl_bloomfilter_amd as mod

    assert mod._lib.load().btlbf_device_count() > 0, "GPU tests need a GPU (and the HIP library)"
    return mod


SEEDS31 = ["1110111011101110111011101110111", "1101101101101101011011011011011"]
# name -> (k, h, spaced seeds, h2).  h <= 4 without seeds: the pipelined incrementMin; h = 5, 8 and seeds: its loop
HASHING = {"h1": (31, 1, None, 1), "h3": (31, 3, None, 1), "h4": (31, 4, None, 1), "h5": (25, 5, None, 1),
           "h8": (31, 8, None, 1), "spaced": (31, 4, SEEDS31, 2)}
# (size, k, h, first RandomState seed whose read is disjoint, 32-bit words of four counters that take more than one
# probe, those of them whose probes come from more than one window).  The first figure is the one usually quoted for
# these seeds (4, 9, 8, 26); at 2^15 one of the eight crowded words holds two probes of a single window, so seven are
# shared BETWEEN windows -- the contention the exact comparison is about.  Both are pinned.
DISJOINT = [(1 << 16, 31, 4, 3, 4, 4), (1 << 16, 25, 5, 33, 9, 9), (1 << 15, 31, 3, 0, 8, 7), (1 << 14, 31, 4, 91, 26, 26)]


@pytest.fixture(scope="module")
def contended(oracle):
    """hashing name -> [(input name, buffer, starts, read_len, clean window offsets, hash rows)], hashed once"""
    cache = {}

    def get(name):
        if name not in cache:
            k, h, seeds, h2 = HASHING[name]
            cache[name] = [(n, buf, st, rl) + m.clean_windows(oracle, buf, k, h, st, rl, seeds, h2)
                           for n, buf, st, rl in m.contended_inputs(11, k, unit=100)]
            for n, buf, st, rl, clean, hv in cache[name]:  # unclean bytes and repeats are really there
                nw = sum(max(e - b - k + 1, 0) for b, e in m.sequences(len(buf), st, rl))
                assert 0 < len(clean) < nw and len(np.unique(hv[:, 0])) < len(clean), n
        return cache[name]

    return get


@pytest.fixture(scope="module")
def disjoint(oracle):
    """row of DISJOINT -> (read, hash rows), with the seed and the word sharing the table states"""
    cache = {}

    def get(case):
        if case not in cache:
            size, k, h, seed, crowded, shared = case
            got, read, hv = m.disjoint_read(oracle, size, k, h)
            pos = m.positions(hv, size)
            assert got == seed and len(hv) == 150 - k + 1 and np.unique(pos).size == pos.size
            assert m.crowded_words(pos, 4) == crowded and m.shared_words(pos, 4) == shared > 0
            assert m.shared_words(pos, 32) > 0  # bit filter: words of 32 positions
            cache[case] = (read, hv)
        return cache[case]

    return get


def new_filter(bf, kind, size, hashing, thr=1):
    k, h, seeds, h2 = HASHING[hashing] if isinstance(hashing, str) else hashing
    f = bf.BloomFilter(size, h, k) if kind == "bits" else bf.CountingBloomFilter(size, h, k, thr)
    if seeds:
        f.setSpacedSeeds(seeds, h2)
    return f


def data_paths(buf, starts, read_len, mis=(0,)):
    """the ways a sequence buffer reaches the kernels -> (label, buffer, starts, read_len): host memory in its own
    layout (at most 65536 bytes without `starts`: the pinned mailbox), host memory with `starts` (staged), a device
    tensor that begins `mis` bytes off alignment"""
    import torch

    a = np.frombuffer(buf, np.uint8).copy()
    yield "host", a, starts, read_len
    if starts is None:
        assert len(buf) <= 65536  # the call above took the mailbox
        yield "host+starts", a, np.array([b for b, _ in m.sequences(len(buf), None, read_len)] + [len(buf)], np.uint64), 0
    for x in mis:
        t = torch.zeros(len(buf) + 16, dtype=torch.uint8, device="cuda")
        t[x:x + len(buf)] = torch.from_numpy(a).cuda()
        ts = None if starts is None else torch.from_numpy(np.asarray(starts).astype(np.int64)).cuda()
        yield "device+%d" % x, t[x:x + len(buf)], ts, read_len


def host(x):
    """an output of a call, wherever it lives -> numpy (bitmaps and counts as uint64)"""
    if isinstance(x, np.ndarray):
        return x
    a = x.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def device_rows(rows):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).cuda()


def bit_oracle(oracle, body, size, h, hv):
    """-> (body after insert of the rows, the serial order's reports)"""
    after = body.copy()
    out = oracle.bf_insert_and_check(after, size, h, hv)
    return after, out


def counter_oracle(oracle, body, h, hv, op):
    after = body.copy()
    (oracle.cbf_increment_all if op == "all" else oracle.cbf_increment_min)(after, h, hv)
    return after


# ---------------------------------------------------------------------------------------------------------------
# BloomFilter: insertAndCheck over sequence buffers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DISJOINT, ids=lambda c: "%d-k%d-h%d" % c[:3])
def test_insert_and_check_seqs_disjoint_read_is_exact(bf, oracle, disjoint, case):
    size, k, h = case[:3]
    read, hv = disjoint(case)
    clean = np.arange(len(hv))
    body = m.prefilled_bits(size + h, size)
    expect, serial = bit_oracle(oracle, body, size, h, hv)
    zero_expect, _ = bit_oracle(oracle, np.zeros_like(body), size, h, hv)
    assert 0 < serial.sum() < len(serial)  # density 1/2: both answers occur
    flt = new_filter(bf, "bits", size, (k, h, None, 1))
    for fresh in (True, False):  # a filter nobody has touched since its (lazy) clear, then an uploaded body
        for label, seq, st, rl in data_paths(read, None, 0, mis=(0, 1, 3)):
            if fresh:
                flt.clear()
            else:
                flt.upload(body)
            hit, valid, cnt = flt.insertAndCheckSeqs(seq, st, rl, want_counts=True)
            out = m.check_window_bitmaps(host(hit), host(valid), host(cnt), len(read), clean)
            assert out.tolist() == ([0] * len(hv) if fresh else serial.tolist()), (label, fresh)
            assert (flt.download() == (zero_expect if fresh else expect)).all(), (label, fresh)
            hit, valid, cnt = flt.insertAndCheckSeqs(seq, st, rl, want_counts=True)  # again: all there
            assert m.check_window_bitmaps(host(hit), host(valid), host(cnt), len(read), clean).all(), label
            assert host(cnt).tolist() == [len(hv)] * 2


@pytest.mark.parametrize("hashing", list(HASHING))
@pytest.mark.parametrize("size", [64, 1000, 1 << 16])
def test_insert_and_check_seqs_contended(bf, oracle, contended, size, hashing):
    h = HASHING[hashing][1]
    body = m.prefilled_bits(size, size)
    inputs = contended(hashing)
    serial = np.concatenate([bit_oracle(oracle, body, size, h, hv)[1] for *_, hv in inputs])
    assert serial.min() == 0 and serial.max() == 1  # both answers occur
    flt = new_filter(bf, "bits", size, hashing)
    for i, (name, buf, starts, read_len, clean, hv) in enumerate(inputs):
        pos = m.positions(hv, size)
        expect, _ = bit_oracle(oracle, body, size, h, hv)
        zero_expect, _ = bit_oracle(oracle, np.zeros_like(body), size, h, hv)
        # every input on every data path, each misalignment on some input, all three on the short one
        for label, seq, st, rl in data_paths(buf, starts, read_len, mis=(0, 1, 3) if name == "tandem" else ((0, 1, 3)[i % 3],)):
            for before, want in ((body, expect), (np.zeros_like(body), zero_expect)):
                if before is body:
                    flt.upload(before)
                else:
                    flt.clear()
                hit, valid, cnt = flt.insertAndCheckSeqs(seq, st, rl, want_counts=True)
                try:
                    out = m.check_window_bitmaps(host(hit), host(valid), host(cnt), len(buf), clean)
                    m.check_bit_insert_and_check(size, before, flt.download(), want, pos, out)
                except m.ContractViolation as e:
                    pytest.fail("%s, %s, %s body: %s" % (name, label, "uploaded" if before is body else "cleared", e))


# ---------------------------------------------------------------------------------------------------------------
# BloomFilter: insertAndCheck over hash rows, parallel order
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [64, 1000, 4096])
def test_bit_insert_and_check_rows_parallel(bf, oracle, size):
    hs = (1, 3, 4, 5, 8)
    body = m.prefilled_bits(size + 1, size)
    rows = {h: m.disjoint_rows(size + h, size, h) for h in hs}
    serial = {h: bit_oracle(oracle, body, size, h, rows[h]) for h in hs}
    both = np.concatenate([serial[h][1] for h in hs])
    assert both.min() == 0 and both.max() == 1
    for h in hs:
        flt = bf.BloomFilter(size, h, 20)
        pos = m.positions(rows[h], size)
        assert np.unique(pos).size == pos.size and (rows[h] >= np.uint64(1 << 63)).any()
        for dev in (False, True):  # disjoint rows: the serial order's answers
            flt.upload(body)
            out = host(flt.insertAndCheck(device_rows(rows[h]) if dev else rows[h], serial=False))
            assert out.tolist() == serial[h][1].tolist(), (h, dev)
            assert (flt.download() == serial[h][0]).all(), (h, dev)
        dup = m.duplicated_rows(size + h, rows[h])
        dpos = m.positions(dup, size)
        for before in (body, np.zeros_like(body)):
            want, _ = bit_oracle(oracle, before, size, h, dup)
            for dev in (False, True):
                flt.upload(before)
                out = host(flt.insertAndCheck(device_rows(dup) if dev else dup, serial=False))
                try:
                    m.check_bit_insert_and_check(size, before, flt.download(), want, dpos, out)
                except m.ContractViolation as e:
                    pytest.fail("h %d, %d duplicated rows, device %s: %s" % (h, len(dup), dev, e))


# ---------------------------------------------------------------------------------------------------------------
# CountingBloomFilter: incrementAll, parallel, always exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [8, 64, 1001, 4096])
def test_increment_all_rows_parallel(bf, oracle, nbytes):
    for h in (1, 3, 4, 8):
        c = bf.CountingBloomFilter(nbytes, h, 20)
        size = c.size()
        assert size == (nbytes + 7) // 8 * 8
        few = size <= 64  # a handful of rows: each often enough to take a counter from 0 to 255
        rows = m.duplicated_rows(nbytes + h, m.disjoint_rows(nbytes + h, size, h), 256 if few else 1, 300 if few else 64)
        prefilled = m.prefilled_counters(nbytes + h, size)
        for before in (prefilled, np.zeros(size, np.uint8)):
            want = counter_oracle(oracle, before, h, rows, "all")
            if few or before is prefilled:
                assert ((before < 255) & (want == 255)).any()  # counters reach 255 inside the call
            for dev in (False, True):
                c.upload(before)
                c.incrementAll(device_rows(rows) if dev else rows)
                m.check_increment_all(c.download(), want)


@pytest.mark.parametrize("mode", ["direct", "partitioned"])
@pytest.mark.parametrize("nbytes", [8, 64, 1001, 4096])
def test_increment_all_seqs_parallel(bf, oracle, contended, nbytes, mode):
    """the planner accepts every one of these sizes (one segment, one level-0 bin): pass C is asserted to have run"""
    for hashing in ("h1", "h4", "h5", "h8"):
        k, h = HASHING[hashing][:2]
        c = new_filter(bf, "counting", nbytes, hashing)
        c.setInsertMode(mode)
        c.setProfiling(True)
        size = c.size()
        prefilled = m.prefilled_counters(nbytes + h, size)
        for i, (name, buf, starts, read_len, clean, hv) in enumerate(contended(hashing)):
            paths = list(data_paths(buf, starts, read_len, mis=((0, 1, 3)[i % 3],)))
            label, seq, st, rl = paths[i % len(paths)]
            # an uploaded body; a freshly created / cleared filter (partitioned: segments built from zero in LDS)
            for before in (prefilled, None):
                if before is None:
                    if i % 2:
                        c.clear()
                    else:
                        c = new_filter(bf, "counting", nbytes, hashing)
                        c.setInsertMode(mode)
                        c.setProfiling(True)
                    before = np.zeros(size, np.uint8)
                else:
                    c.upload(before)
                want = counter_oracle(oracle, before, h, hv, "all")
                if name.startswith("repeat"):
                    assert ((before < 255) & (want == 255)).any()
                c.getProfile()
                c.insertSeqs(seq, st, rl, increment_all=True)
                prof = c.getProfile()
                try:
                    m.check_increment_all(c.download(), want)
                except m.ContractViolation as e:
                    pytest.fail("%s, %s, %s, %s: %s" % (hashing, name, label, "uploaded" if before is prefilled else "fresh", e))
                assert ("insert_apply" in prof) == (mode == "partitioned"), (hashing, name, prof)


# ---------------------------------------------------------------------------------------------------------------
# CountingBloomFilter: incrementMin, parallel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", range(1, 9))
@pytest.mark.parametrize("nbytes", [8, 64])
def test_increment_min_one_window_per_call_is_exact(bf, oracle, nbytes, h):
    # no concurrency at all: what is left is a window whose own probes collide in one byte and in one word
    k = 25
    rng = np.random.RandomState(nbytes + h)
    kmers = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for _ in range(120)]
    calls = [kmers[i] for i in rng.randint(0, len(kmers), 200)]
    rows = [oracle.nthash_seq(s, h, k)[1] for s in calls]
    pos = [m.positions(hv, nbytes)[0].tolist() for hv in rows]
    assert all(len(p) == h for p in pos)
    if h > 1:  # two probes of a window in one byte, and in two bytes of one word
        assert any(len(set(p)) < h for p in pos) and any(len({x // 4 for x in p}) < len(set(p)) for p in pos)
    c = bf.CountingBloomFilter(nbytes, h, k)
    mine = m.prefilled_counters(h, nbytes) if h % 2 else np.zeros(nbytes, np.uint8)
    c.upload(mine)
    for call, (s, hv) in enumerate(zip(calls, rows)):
        oracle.cbf_increment_min(mine, h, hv)
        c.insertSeqs(s)
        if call % 50 == 49:
            assert (c.download() == mine).all(), call


@pytest.mark.parametrize("case", DISJOINT, ids=lambda c: "%d-k%d-h%d" % c[:3])
def test_increment_min_disjoint_read_is_exact(bf, oracle, disjoint, case):
    # no two windows share a counter, so the order cannot matter -- but windows do share words, so the word
    # compare-and-swap behind every byte update is contended all the same
    size, k, h = case[:3]
    read, hv = disjoint(case)
    c = bf.CountingBloomFilter(size, h, k)
    for before in (np.zeros(size, np.uint8), m.prefilled_counters(size + h, size)):
        want = counter_oracle(oracle, before, h, hv, "min")
        for label, seq, st, rl in data_paths(read, None, 0, mis=(0, 1, 3)):
            c.upload(before)
            c.insertSeqs(seq, st, rl)
            got = c.download()
            assert (got == want).all(), (label, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("nbytes", [64, 1001, 4096])
def test_increment_min_disjoint_rows_are_exact(bf, oracle, nbytes):
    for h in (1, 3, 4, 5, 8):
        c = bf.CountingBloomFilter(nbytes, h, 20)
        size = c.size()
        rows = m.disjoint_rows(nbytes + h, size, h)
        before = m.prefilled_counters(nbytes + h, size)
        want = counter_oracle(oracle, before, h, rows, "min")
        assert (want != before).any() and (rows >= np.uint64(1 << 63)).any()
        for dev in (False, True):
            c.upload(before)
            c.incrementMin(device_rows(rows) if dev else rows)
            got = c.download()
            assert (got == want).all(), (h, dev, np.flatnonzero(got != want)[:5])


@pytest.mark.parametrize("hashing", ["h3", "h4", "h5", "h8", "spaced"])
@pytest.mark.parametrize("nbytes", [64, 4096])
def test_increment_min_contended(bf, oracle, contended, nbytes, hashing):
    h = HASHING[hashing][1]
    c = new_filter(bf, "counting", nbytes, hashing)
    prefilled = m.prefilled_counters(nbytes + h, nbytes)
    for i, (name, buf, starts, read_len, clean, hv) in enumerate(contended(hashing)):
        pos = m.positions(hv, nbytes)
        for before in (np.zeros(nbytes, np.uint8), prefilled):
            upper = counter_oracle(oracle, before, h, hv, "all")
            if name == "tandem" and before is not prefilled:
                assert upper.max() < 255  # M4 is in force on this one
            if name.startswith("repeat"):
                assert upper.max() == 255
            for label, seq, st, rl in data_paths(buf, starts, read_len, mis=((0, 1, 3)[i % 3],)):
                c.upload(before)
                c.insertSeqs(seq, st, rl)
                try:
                    m.check_increment_min(before, c.download(), upper, pos)
                except m.ContractViolation as e:
                    pytest.fail("%s, %s, %s body: %s" % (name, label, "prefilled" if before is prefilled else "zero", e))


# ---------------------------------------------------------------------------------------------------------------
# CountingBloomFilter: insertAndCheck over hash rows, parallel order
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [1, 2, 255])
@pytest.mark.parametrize("nbytes", [64, 1001, 4096])
def test_counting_insert_and_check_rows_parallel(bf, oracle, nbytes, thr):
    hs = (1, 3, 4, 8)
    size = (nbytes + 7) // 8 * 8
    disjoint_rows = {h: m.disjoint_rows(nbytes + h, size, h) for h in hs}
    bodies = {h: m.prefilled_counters(nbytes + h + thr, size) for h in hs}
    after = {h: bodies[h].copy() for h in hs}
    reports = {h: oracle.cbf_insert_and_check(after[h], h, thr, disjoint_rows[h]) for h in hs}
    both = np.concatenate([reports[h] for h in hs])
    assert both.min() == 0 and both.max() == 1  # both answers occur
    for h in hs:
        c = bf.CountingBloomFilter(nbytes, h, 20, thr)
        assert c.size() == size
        rows, prefilled, want, serial = disjoint_rows[h], bodies[h], after[h], reports[h]
        for dev in (False, True):  # disjoint rows: the serial order's answers and counters
            c.upload(prefilled)
            out = host(c.insertAndCheck(device_rows(rows) if dev else rows, serial=False))
            assert out.tolist() == serial.tolist(), (h, dev)
            assert (c.download() == want).all(), (h, dev)
        dup = m.duplicated_rows(nbytes + h, rows)
        dpos = m.positions(dup, size)
        for before in (prefilled, np.zeros(size, np.uint8)):
            upper = counter_oracle(oracle, before, h, dup, "all")
            for dev in (False, True):
                c.upload(before)
                out = host(c.insertAndCheck(device_rows(dup) if dev else dup, serial=False))
                try:
                    m.check_counting_insert_and_check(before, c.download(), upper, dpos, out, thr)
                except m.ContractViolation as e:
                    pytest.fail("h %d, %d duplicated rows, device %s: %s" % (h, len(dup), dev, e))


# ---------------------------------------------------------------------------------------------------------------
# CountingBloomFilter: minCount over sequence buffers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hashing", ["h3", "h5", "spaced"])
def test_min_count_seqs_vs_oracle(bf, oracle, contended, hashing):
    h = HASHING[hashing][1]
    c = new_filter(bf, "counting", 1001, hashing, thr=2)
    size = c.size()
    assert size == 1008
    body = m.prefilled_counters(h, size)
    c.upload(body)
    for i, (name, buf, starts, read_len, clean, hv) in enumerate(contended(hashing)):
        mn, _ = oracle.cbf_query(body, h, 2, hv)
        want = np.zeros(len(buf), np.uint8)  # 0 at unclean windows and past a sequence's last window
        want[clean] = mn
        assert len(set(mn.tolist())) > 2
        for label, seq, st, rl in data_paths(buf, starts, read_len, mis=(0, 1, 3)):
            got, valid = c.minCountSeqs(seq, st, rl)
            assert (host(got) == want).all(), (name, label, np.flatnonzero(host(got) != want)[:5])
            m.check_window_bitmaps(np.zeros_like(host(valid)), host(valid), None, len(buf), clean)
    assert (c.download() == body).all()


def test_min_count_seqs_on_a_shard_is_einval(bf):
    # a counting shard has no Python class of its own: the C ABI directly, on a handle this test owns
    L, lib = bf._lib.load(), bf._lib
    hnd = C.c_void_p()
    lib.check(L.btlbf_create_shard(C.byref(hnd), lib.COUNTING8, 1024, 1, 2, 3, 25, 1, 0))
    try:
        seq = np.frombuffer(b"ACGT" * 20, np.uint8).copy()
        mn, valid = np.zeros(seq.size, np.uint8), np.zeros(2, np.uint64)
        rc = L.btlbf_min_count_seqs(hnd, C.c_void_p(seq.ctypes.data), seq.size, None, C.c_void_p(mn.ctypes.data),
                                    C.c_void_p(valid.ctypes.data), lib.HOST, None)
        assert rc == lib.EINVAL and not mn.any() and not valid.any()
        rows, out = np.arange(6, dtype=np.uint64), np.zeros(2, np.uint8)
        rc = L.btlbf_insert_and_check_hashes(hnd, C.c_void_p(rows.ctypes.data), 2, C.c_void_p(out.ctypes.data),
                                             lib.ORDER_PARALLEL, lib.HOST, None)  # needs all h probes of a k-mer as well
        assert rc == lib.EINVAL
    finally:
        L.btlbf_destroy(hnd)
