"""The k-mer cardinality sketch on the GPU (btlbf_card_* through engine.KmerCardinality) against the numpy model
(tests/cardinality_model.py): the table and the three totals are equal to the model's bit for bit.

  shapes       k in {4, 25, 31, 32, 33, 64} x (sample_bits, table_bits) in {(0, 6), (0, 10), (1, 8), (3, 10), (11, 12)} --
               at table_bits 6 every window collides in 64 counters (the atomics), at sample_bits 11 hardly anything is
               sampled (the mask) -- over three inputs: one sequence of 5 000 bases without a layout (it crosses the tile
               of 2 048 window starts twice), 64 rows of 100 (read_len), and a ragged buffer with an empty sequence, one of
               k - 1 and one of k bases, lowercase, U, N at the start, in the middle and at the end, and a sequence longer
               than a tile; from host memory and from device memory on a non-blocking stream on which the copy of the
               input is still queued behind a delay when the call is issued (the buffer holds other, valid reads until then)
  accumulation two calls over halves equal one; merge equals the sketch of both inputs; clear zeroes everything
  saturation   counters uploaded at 2^32 - 3, 2^32 - 2 and 2^32 - 1 stop at 2^32 - 1, their neighbours are exact; merge
               saturates too
  histogram    np.bincount of the downloaded table folded at n_hist - 1, n_hist in {3, 64, 8192}, also on an uploaded table
               with counts from 0 to 10 000 and saturated counters
  estimate     estimate_now on the accuracy input (test_cardinality_solve_cpu.py) equals the model's solve to 1e-9 and so
               lies within that test's caps
  poison       t, f, est, table and totals3 pre-filled with a poison byte: every byte is overwritten"""
import ctypes as C

import numpy as np
import pytest

import cardinality_model as M
from poison import POISONS, Poison, assert_same
from test_gpu_auto_query import bf  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

KS = [4, 25, 31, 32, 33, 64]
SR = [(0, 6), (0, 10), (1, 8), (3, 10), (11, 12)]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def bases(rng, n):
    return rng.choice(ACGT, n).astype(np.uint8)


def make_inputs(k):
    """name -> (buffer, starts or None, read_len)"""
    rng = np.random.RandomState(1000 + k)
    one = bases(rng, 5000)
    rows = bases(rng, 64 * 100)
    lower = np.frombuffer(bytes(bases(rng, 200)).lower(), np.uint8).copy()
    with_u = bases(rng, 150)
    with_u[with_u == ord("T")] = ord("U")
    with_u[5] = ord("u")
    n_start, n_mid, n_end = bases(rng, 120), bases(rng, 300), bases(rng, 130)
    n_start[0] = n_mid[150] = n_mid[151] = n_end[-1] = ord("N")
    seqs = [bases(rng, 90), np.zeros(0, np.uint8), bases(rng, k - 1), bases(rng, k), lower, with_u, n_start, n_mid, n_end,
            bases(rng, 2048 + k + 50), np.zeros(0, np.uint8), bases(rng, k + 1)]
    starts = np.concatenate([[0], np.cumsum([s.size for s in seqs])]).astype(np.uint64)
    return {"one": (one, None, 0), "rows": (rows, None, 100), "ragged": (np.concatenate(seqs), starts, 0)}


@pytest.fixture(scope="module")
def hashed(oracle):
    """k -> name -> (buffer, starts, read_len, windows, hashes): the model's hashes, computed once per k and input"""
    out = {}
    for k in KS:
        out[k] = {}
        for name, (buf, starts, read_len) in make_inputs(k).items():
            w, h = M.window_hashes(oracle, buf, k, starts, read_len)
            out[k][name] = (buf, starts, read_len, w, h)
    return out


def got(c):
    t, n = c._download()
    return t, n


def same(note, c, want):
    t, n = got(c)
    wt, wn = want
    assert list(n) == list(wn), "%s: totals %s, expected %s" % (note, list(n), list(wn))
    bad = np.flatnonzero(t != wt)
    assert bad.size == 0, "%s: %d counters differ, the first at %d: %d, expected %d" % (note, bad.size, bad[0], t[bad[0]],
                                                                                      wt[bad[0]])


def add_late(c, buf, starts, read_len):
    """addSeqs from device memory on a non-blocking stream: the buffer (and its offsets) hold a decoy -- other valid reads,
    other valid offsets with the same ends -- until copies queued on that stream behind a delay bring the real input"""
    import torch

    s = torch.cuda.Stream()
    src = torch.from_numpy(buf.copy()).pin_memory()
    dst = torch.from_numpy(buf[::-1].copy()).cuda()
    src_st = dst_st = None
    if starts is not None:
        src_st = torch.from_numpy(starts.view(np.int64).copy()).pin_memory()
        decoy = np.full(starts.size, starts[-1], np.uint64)
        decoy[0] = 0
        dst_st = torch.from_numpy(decoy.view(np.int64)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(2_000_000)
        dst.copy_(src, non_blocking=True)
        if starts is not None:
            dst_st.copy_(src_st, non_blocking=True)
        c.addSeqs(dst, starts=dst_st, read_len=read_len)  # torch's current stream: s
    s.synchronize()


@pytest.mark.parametrize("s,r", SR, ids=["s%dr%d" % sr for sr in SR])
@pytest.mark.parametrize("k", KS)
def test_table_and_totals_equal_the_model(bf, hashed, k, s, r):  # noqa: F811
    c = bf.KmerCardinality(k, s, r)
    try:
        for name, (buf, starts, read_len, w, h) in hashed[k].items():
            want = M.add(*M.empty(r), w, h, s, r)
            if s == 0:
                assert want[1][2] == want[1][1] > 0
            c.addSeqs(buf, starts=starts, read_len=read_len)
            same("k=%d s=%d r=%d %s host" % (k, s, r, name), c, want)
            c.clear()
            add_late(c, buf, starts, read_len)
            same("k=%d s=%d r=%d %s device" % (k, s, r, name), c, want)
            c.clear()
    finally:
        c.close()


def test_the_model_samples_what_the_shapes_are_for(hashed):
    """the cases test what they say: at sample_bits 11 a few windows are sampled, not none; at table_bits 6 every counter
    is hit many times"""
    sampled = sum(M.buckets(h, 11, 12).size for k in KS for (_, _, _, _, h) in hashed[k].values())
    assert 0 < sampled < 200, sampled
    t, _ = M.add(*M.empty(6), *hashed[25]["one"][3:], 0, 6)
    assert t.min() > 30


def test_two_calls_over_halves_equal_one_and_clear_zeroes(bf, hashed):  # noqa: F811
    buf, _, read_len, w, h = hashed[25]["rows"]
    want = M.add(*M.empty(10), w, h, 0, 10)
    c = bf.KmerCardinality(25, 0, 10)
    c.addSeqs(buf[: 32 * 100], read_len=read_len)
    assert c.totals()[0] == w // 2
    c.addSeqs(buf[32 * 100:], read_len=read_len)
    same("two halves", c, want)
    c.clear()
    same("cleared", c, M.empty(10))
    c.addSeqs(buf, read_len=read_len)
    same("after the clear", c, want)
    c.close()


def test_merge_equals_the_sketch_of_both_inputs(bf, hashed):  # noqa: F811
    (b1, _, _, w1, h1), (b2, st2, _, w2, h2) = hashed[31]["one"], hashed[31]["ragged"]
    a, b = bf.KmerCardinality(31, 1, 8), bf.KmerCardinality(31, 1, 8)
    a.addSeqs(b1)
    b.addSeqs(b2, starts=st2)
    want_b = M.add(*M.empty(8), w2, h2, 1, 8)
    want = M.add(*want_b, w1, h1, 1, 8)
    assert (M.merge(M.add(*M.empty(8), w1, h1, 1, 8), want_b)[0] == want[0]).all()
    assert a.merge(b) is a
    same("merged", a, want)
    same("the source of a merge", b, want_b)
    other = bf.KmerCardinality(31, 1, 9)
    with pytest.raises(bf._lib.BtlbfError) as e:
        a.merge(other)
    assert e.value.code == bf._lib.EINVAL
    same("after a refused merge", a, want)
    for x in (a, b, other):
        x.close()


def test_counters_saturate_and_never_wrap(bf, hashed):  # noqa: F811
    buf, _, read_len, w, h = hashed[25]["rows"]
    r = 6
    inc = np.bincount(M.buckets(h, 0, r), minlength=1 << r)
    assert inc.min() >= 3  # every counter takes at least three increments
    table = np.zeros(1 << r, np.uint32)
    table[[10, 11, 12]] = [M.SAT - 2, M.SAT - 1, M.SAT]
    table[[40, 42]] = [M.SAT - int(inc[40]), M.SAT - int(inc[42]) - 1]  # ends exactly at the maximum; one below it
    tot = np.array([5, 4, 3], np.uint64)
    want = M.add(table, tot, w, h, 0, r)
    assert list(want[0][[10, 11, 12, 40, 42]]) == [M.SAT] * 4 + [M.SAT - 1] and want[0][9] == inc[9] and want[0][13] == inc[13]
    c = bf.KmerCardinality(25, 0, r)
    c.upload(table, tot)
    same("uploaded", c, (table, tot))
    c.addSeqs(buf, read_len=read_len)
    same("saturated", c, want)
    c.addSeqs(buf, read_len=read_len)  # ... and they stay there
    same("saturated, added again", c, M.add(*want, w, h, 0, r))
    d = bf.KmerCardinality(25, 0, r)
    d.upload(table, tot)
    c.merge(d)
    same("merged into saturated counters", c, M.merge(M.add(*want, w, h, 0, r), (table, tot)))
    c.close()
    d.close()


@pytest.mark.parametrize("n_hist", [3, 64, 8192])
def test_histogram_equals_bincount(bf, hashed, n_hist):  # noqa: F811
    buf, _, _, w, h = hashed[25]["one"]
    c = bf.KmerCardinality(25, 0, 10)
    c.addSeqs(buf)
    t = c.histogram(n_hist)
    assert t.sum() == 1 << 10 and (t == M.histogram(c.table(), n_hist)).all()
    assert (t == M.histogram(M.add(*M.empty(10), w, h, 0, 10)[0], n_hist)).all()
    c.close()
    # counts from 0 to 10 000, saturated counters, and nearly everything zero (the ballot's path) in a table of several
    # workgroups
    r = 16
    table = np.zeros(1 << r, np.uint32)
    rng = np.random.RandomState(5)
    idx = rng.permutation(1 << r)[:20000]
    table[idx[:10001]] = np.arange(10001)
    table[idx[10001:10011]] = M.SAT
    table[idx[10011:]] = rng.randint(1, 4, idx.size - 10011)
    c = bf.KmerCardinality(25, 3, r)
    c.upload(table, np.zeros(3, np.uint64))
    t = c.histogram(n_hist)
    want = M.histogram(table, n_hist)
    assert t.size == n_hist and (t == want).all(), np.flatnonzero(t != want)[:5]
    c.close()


@pytest.mark.parametrize("s,r", [(0, 18), (2, 16)])
def test_estimate_on_the_accuracy_input_equals_the_models_solve(bf, oracle, s, r):  # noqa: F811
    w, h = M.accuracy_hashes(oracle)
    c = bf.KmerCardinality(M.ACC_K, s, r)
    c.addSeqs(M.accuracy_reads(), read_len=M.ACC_LEN)
    want_table, want_tot = M.add(*M.empty(r), w, h, s, r)
    same("accuracy input", c, (want_table, want_tot))
    e = c.estimate(64)
    F0, f, occ = M.solve(M.histogram(want_table, 64), s, r)
    close = lambda a, b: abs(a - b) <= 1e-9 * max(abs(b), F0)
    assert close(e.distinct, F0) and close(e.singletons, f[1]) and close(e.occupancy, occ)
    assert e.spectrum.size == 62 and all(close(a, b) for a, b in zip(e.spectrum, f[1:]))
    assert (e.windows, e.clean_windows, e.sampled) == tuple(int(x) for x in want_tot)
    assert close(e.at_least(3), F0 - f[1] - f[2])
    distinct, once = M.accuracy_truth(oracle)
    print("s=%d r=%d: F0 %.1f of %d (%+.2f %%), f1 %.1f of %d (%+.2f %%), occupancy %.3f"
          % (s, r, e.distinct, distinct, 100 * (e.distinct / distinct - 1), e.singletons, once,
             100 * (e.singletons / once - 1), e.occupancy))
    assert abs(e.distinct / distinct - 1) <= (0.02 if s == 0 else 0.05)
    if s == 0:
        assert abs(e.singletons / once - 1) <= 0.03
    c.close()


@pytest.mark.parametrize("byte", POISONS)
def test_every_output_byte_is_written(bf, hashed, byte):  # noqa: F811
    L = bf._lib
    lib = L.load()
    buf, _, read_len, w, h = hashed[25]["rows"]
    r, s, n_hist = 12, 1, 16  # (some 2 400 sampled windows in 4 096 counters: the table is not full)
    want_table, want_tot = M.add(*M.empty(r), w, h, s, r)
    assert 0 < (want_table == 0).sum() < want_table.size
    c = bf.KmerCardinality(25, s, r)
    c.addSeqs(buf, read_len=read_len)
    reg = Poison(byte)
    table, p_table = reg.alloc(1 << r, np.uint32, name="table")
    tot, p_tot = reg.alloc(3, np.uint64, name="totals3")
    assert lib.btlbf_card_download(c._h, p_table, p_tot) == L.OK
    assert_same("table", table, want_table)
    assert_same("totals3", tot, want_tot)
    t, p_t = reg.alloc(n_hist, np.uint64, name="t")
    assert lib.btlbf_card_histogram(c._h, p_t, n_hist) == L.OK
    want_t = M.histogram(want_table, n_hist)
    assert_same("t", t, want_t)
    F0, f, occ = M.solve(want_t, s, r)
    for call in ("estimate_now", "solve"):
        est, p_est = reg.alloc(C.sizeof(L.CardEstimate), np.uint8, name="est")
        fo, p_f = reg.alloc(n_hist - 1, np.float64, name="f")
        if call == "solve":
            rc = lib.btlbf_card_solve(p_t, n_hist, s, r, C.cast(p_est, C.POINTER(L.CardEstimate)), p_f)
        else:
            rc = lib.btlbf_card_estimate_now(c._h, n_hist, C.cast(p_est, C.POINTER(L.CardEstimate)), p_f)
        assert rc == L.OK
        e = L.CardEstimate.from_buffer_copy(est.tobytes())
        assert abs(e.distinct - F0) <= 1e-9 * F0 and abs(e.occupancy - occ) <= 1e-9 and e.overflow_buckets == want_t[-1]
        assert (e.windows, e.clean_windows, e.sampled) == (tuple(int(x) for x in want_tot) if call == "estimate_now" else (0, 0, 0))
        assert fo[0] == 0.0 and np.all(np.abs(fo - f) <= 1e-9 * F0), (fo, f)
        assert not np.isnan(fo).any()
    reg.check_guards()
    c.close()
