"""The 16-, 32- and 64-bit counting filters (csrc/wide_counter_kernels.hip, csrc/wide_counter.hpp) under contention:
the wide counterpart of tests/test_gpu_update_order.py, on its inputs.  Every update of tests/test_gpu_wide_counters.py
is some 400 bytes in one tile of one workgroup; here one call spans 15 to 35 tiles and as many workgroups whose lanes
fight over the same counters -- and, at 16 bits, over the two halves of the same 32-bit words -- read boundaries move
from tile to tile (2048 % 100 = 48), windows straddle tile boundaries, and 16-bit counters saturate from the call's own
increments.

incrementAll in parallel order is exact (A1); incrementMin obeys M1-M4 of tests/wide_counter_model.py, which
tests/test_wide_update_order_cpu.py shows to accept every schedule of the correct algorithm and to reject the usual
mistakes; the serial order and every query are exact.  Every comparison is integer-exact or one of those stated
inequalities.  The conditions under which a case means something are asserted on oracle and model data before the GPU
call; contention comes from the inputs of one call, nothing is run in a loop."""
import numpy as np
import pytest

import poison
import update_order_model as uo
import wide_counter_model as wm
import wide_update_order_model as w

pytestmark = pytest.mark.gpu
WIDTHS = (16, 32, 64)
SEEDS31 = ["1110111011101110111011101110111", "1101101101101101011011011011011"]
# name -> (k, h, spaced seeds, h2): tests/test_gpu_update_order.py's HASHING and h = 2.  Queries: h <= 4 without seeds
# take the pipelined path, whose `i < h` guards h = 1, 2 and 4 exercise; h = 5 and 8 the plain loop; seeds the walk
HASHING = {"h1": (31, 1, None, 1), "h2": (31, 2, None, 1), "h3": (31, 3, None, 1), "h4": (31, 4, None, 1),
           "h5": (25, 5, None, 1), "h8": (31, 8, None, 1), "spaced": (31, 4, SEEDS31, 2)}
SIZES = (8, 64, 1000, 4096)  # bytes: 4 / 2 / 1 counters .. 2048 / 1024 / 512
# clean windows that start in the last k - 1 offsets of a 2048-window tile, by k: figures of the inputs, evaluated with
# the oracle on a CPU and pinned (the windows do not depend on the hash count)
STRADDLING = {31: {"repeat300": 286, "repeat700": 668, "ragged6": 3}, 25: {"repeat300": 156, "repeat700": 380, "ragged6": 30}}
MULTI_TILE = ("repeat300", "repeat700", "ragged6")


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    from btl_bloomfilter_amd import engine

    return engine


@pytest.fixture(scope="module")
def contended(oracle):
    """hashing name -> [(input name, buffer, starts, read_len, clean window offsets, hash rows)], hashed once: the inputs
    of tests/test_gpu_update_order.py with 700 copies for 600 (70,000 bytes: above the 65,536 of the pinned mailbox) and
    the ragged list six times over"""
    cache = {}

    def get(name):
        if name not in cache:
            k, h, seeds, h2 = HASHING[name]
            inputs = uo.contended_inputs(11, k, unit=100, repeats=(300, 700))
            assert [x[0] for x in inputs] == ["tandem", "repeat300", "repeat700", "ragged"]
            inputs.append(("ragged6",) + w.enlarged_ragged(11, inputs[3][1], inputs[3][2]) + (0,))
            cache[name] = [(n, buf, st, rl) + uo.clean_windows(oracle, buf, k, h, st, rl, seeds, h2) for n, buf, st, rl in inputs]
            for n, buf, st, rl, clean, hv in cache[name]:
                nw = sum(max(e - b - k + 1, 0) for b, e in uo.sequences(len(buf), st, rl))
                assert 0 < len(clean) < nw and len(np.unique(hv[:, 0])) < len(clean), n  # unclean bytes, repeated k-mers
                tiles = (len(buf) + w.TILE - 1) // w.TILE
                if n in MULTI_TILE:
                    assert tiles >= 5 and w.straddling(clean, k) == STRADDLING[k][n] > 0, (n, tiles, w.straddling(clean, k))
                else:
                    assert tiles == 1
            assert len(inputs[1][1]) == 30000 and len(inputs[2][1]) == 70000 > 65536
            assert (len(inputs[1][1]) + w.TILE - 1) // w.TILE == 15 and (len(inputs[2][1]) + w.TILE - 1) // w.TILE == 35
        return cache[name]

    return get


@pytest.fixture(scope="module")
def probes(contended):
    """(hashing, counters) -> the positions of every input's clean windows, reduced once"""
    cache = {}

    def get(hashing, size):
        if (hashing, size) not in cache:
            cache[hashing, size] = [uo.positions(hv, size) for *_, hv in contended(hashing)]
        return cache[hashing, size]

    return get


def body_of(bits, nbytes):
    n = wm.round_bytes(nbytes) * 8 // bits
    raw = wm.prefilled_body(bits, n, 11)
    return np.frombuffer(raw, np.uint8), np.frombuffer(raw, wm.DTYPES[bits]).astype(np.uint64)


def new_filter(eng, bits, nbytes, hashing, thr=1):
    k, h, seeds, h2 = HASHING[hashing]
    f = eng.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
    if seeds:
        f.setSpacedSeeds(seeds, h2)
    assert f.size() == wm.round_bytes(nbytes) * 8 // bits
    return f


def device_slice(a, off):
    """a 1-D slice buf_dev[off:] of a padded tensor: its address is `off` bytes past an aligned one"""
    import torch

    t = torch.zeros(off + len(a) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[off:off + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    s = t[off:off + len(a)]
    assert s.data_ptr() % 4 == off and s.is_contiguous()
    return s


def explicit_starts(n_bytes, read_len):
    return np.array([b for b, _ in uo.sequences(n_bytes, None, read_len)] + [n_bytes], np.uint64)


def data_paths(name, buf, starts, read_len, turn, other_layout):
    """the ways a sequence buffer reaches the kernels -> (label, buffer, starts, read_len): host memory, and a device
    tensor 1, 2 or 3 bytes off alignment (`turn` picks which; the one-tile tandem input takes all three).  A uniform
    buffer comes under read_len and, with other_layout, once more under explicit starts (from host memory on even turns,
    from the device on odd ones)"""
    import torch

    a = np.frombuffer(buf, np.uint8).copy()
    yield "host", a, starts, read_len
    both = read_len and other_layout
    st2 = explicit_starts(len(buf), read_len) if both else None
    if both and turn % 2 == 0:
        yield "host+starts", a, st2, 0
    for off in (1, 2, 3) if name == "tandem" else (1 + turn % 3,):
        d = device_slice(a, off)
        ts = None if starts is None else torch.from_numpy(np.asarray(starts).astype(np.int64)).cuda()
        yield "device+%d" % off, d, ts, read_len
        if both and turn % 2 == 1:
            yield "device+%d+starts" % off, d, torch.from_numpy(st2.astype(np.int64)).cuda(), 0


def turn_of(bits, hashing, nbytes):
    return WIDTHS.index(bits) + list(HASHING).index(hashing) + SIZES.index(nbytes)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# updates in parallel order
# ---------------------------------------------------------------------------------------------------------------
def run_updates(eng, contended, probes, bits, hashing, nbytes, ops, names, one_path):
    """the inputs `names` through incrementAll (exact) and / or incrementMin (M1-M4) on the prefilled filter, on every
    data path, or, with one_path, on one that the case's turn picks"""
    mx = wm.max_of(bits)
    raw, before = body_of(bits, nbytes)
    f = new_filter(eng, bits, nbytes, hashing)
    size = f.size()
    turn = turn_of(bits, hashing, nbytes)
    for i, ((name, buf, starts, read_len, clean, hv), pos) in enumerate(zip(contended(hashing), probes(hashing, size))):
        if name not in names:
            continue
        upper = wm.increment_all_exact(before, pos, mx)
        # -- the conditions, on model data --
        assert (uo._windows_per_position(pos, size) > 1).any(), name  # a counter that several windows probe
        if bits == 16:
            assert uo.shared_words(pos, 2) > 0, name  # words whose two halves belong to different windows
        if name == "repeat700":
            if bits == 16 and nbytes == 64:
                assert uo.shared_words(pos, 2) == 16  # every word of the filter
            if nbytes >= 64:  # a carry out of the low byte and a saturation inside the call
                assert ((before <= 255) & (upper > 255)).any() and ((before != mx) & (upper == mx)).any()
            if (bits, nbytes, hashing) == (16, 8, "h8"):  # 0xffff from the call's own 65,000+ increments
                assert int(((before <= 0x100) & (upper == mx)).sum()) == 4 and np.bincount(pos.ravel()).min() > 65000
        paths = list(data_paths(name, buf, starts, read_len, turn + i, True))
        if one_path:
            paths = [paths[(turn + i) % len(paths)]]
        for label, seq, st, rl in paths:
            if "all" in ops:
                f.upload(raw)
                f.insertSeqs(seq, st, rl, increment_all=True)
                try:
                    wm.check_increment_all(f.counters(), upper)
                except uo.ContractViolation as e:
                    pytest.fail("incrementAll, %s, %s: %s" % (name, label, e))
            if "min" in ops:
                f.upload(raw)
                f.insertSeqs(seq, st, rl)
                try:
                    wm.check_increment_min(before, f.counters(), upper, pos, mx)
                except uo.ContractViolation as e:
                    pytest.fail("incrementMin, %s, %s: %s" % (name, label, e))
    f.close()


ALL_INPUTS = ("tandem", "repeat300", "repeat700", "ragged", "ragged6")


@pytest.mark.parametrize("nbytes", SIZES[1:])
@pytest.mark.parametrize("hashing", list(HASHING))
@pytest.mark.parametrize("bits", WIDTHS)
def test_updates_in_parallel_order(eng, contended, probes, bits, hashing, nbytes):
    run_updates(eng, contended, probes, bits, hashing, nbytes, ("all", "min"), ALL_INPUTS, False)


# On the 8-byte filter -- 4, 2 or 1 counters -- every increment of a call is a compare-and-swap on the same one or two
# words, retried until it wins: a call over repeat700 with eight hashes makes 369,600 of them and takes seconds at 64
# bits.  So that a case stays at a few seconds, each operation and each repeat input is a case of its own there and goes
# by one data path, which the case's turn picks; the one-tile and ragged inputs go by every path.
@pytest.mark.parametrize("names", [("tandem", "ragged", "ragged6"), ("repeat300",), ("repeat700",)], ids=lambda n: n[-1])
@pytest.mark.parametrize("hashing", list(HASHING))
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("op", ["all", "min"])
def test_updates_in_parallel_order_on_the_8_byte_filter(eng, contended, probes, op, bits, hashing, names):
    run_updates(eng, contended, probes, bits, hashing, 8, (op,), names, len(names) == 1)


# ---------------------------------------------------------------------------------------------------------------
# the serial order over valid bits that span tiles
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["min", "all"])
@pytest.mark.parametrize("nbytes", [64, 1000])
@pytest.mark.parametrize("bits", [16, 64])
def test_serial_order_on_the_smallest_multi_tile_input(eng, contended, bits, nbytes, op):
    k, h, _, _ = HASHING["h3"]
    name, buf, starts, read_len, clean, hv = contended("h3")[1]
    assert name == "repeat300" and len(clean) < len(buf) - k + 1
    raw, before = body_of(bits, nbytes)
    model = wm.WideCBF(bits, nbytes, h, k, 1, raw.tobytes())
    for row in hv:
        (model.increment_min if op == "min" else model.increment_all)(row)
    f = new_filter(eng, bits, nbytes, "h3")
    for label, seq, st, rl in data_paths(name, buf, starts, read_len, WIDTHS.index(bits) + (op == "all"), False):
        f.upload(raw)
        f.insertSeqs(seq, st, rl, increment_all=op == "all", serial=True)
        poison.assert_same("%s, serial, %s" % (op, label), f.download(), np.frombuffer(model.body(), np.uint8))
    f.close()


# ---------------------------------------------------------------------------------------------------------------
# queries on the prefilled filter
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("hashing", list(HASHING))
@pytest.mark.parametrize("bits", WIDTHS)
def test_queries_on_the_prefilled_filter(eng, contended, probes, bits, hashing, nbytes):
    mx = wm.max_of(bits)
    raw, before = body_of(bits, nbytes)
    thresholds = (0, 1, 256, min(mx, 0xffffffff))
    filters = [new_filter(eng, bits, nbytes, hashing, thr) for thr in thresholds]
    for f in filters:
        f.upload(raw)
    size = filters[0].size()
    inputs, all_pos = contended(hashing), probes(hashing, size)
    turn = turn_of(bits, hashing, nbytes)
    seen = set()
    for i, ((name, buf, starts, read_len, clean, hv), pos) in enumerate(zip(inputs, all_pos)):
        n = len(buf)
        mins = before[pos].min(axis=1)
        seen |= set(mins.tolist())
        exp_min = np.zeros(n, np.uint64)  # 0 at unclean windows and past a sequence's last window
        exp_min[clean] = mins
        valid = np.zeros(n, bool)
        valid[clean] = True
        for label, seq, st, rl in data_paths(name, buf, starts, read_len, turn + i, False):
            what = "%s, %s" % (name, label)
            for thr, f in zip(thresholds, filters):
                hit, vb, cnt = f.containsSeqs(seq, st, rl, want_counts=True)
                exp_hit = valid & (exp_min >= np.uint64(thr))
                poison.assert_bitmap("hit bits, threshold %d, %s" % (thr, what), hit, exp_hit, n)
                poison.assert_bitmap("valid bits, threshold %d, %s" % (thr, what), vb, valid, n)
                assert host(cnt).view(np.uint64).tolist() == [int(valid.sum()), int(exp_hit.sum())], (thr, what)
            mn, vb = filters[i % len(filters)].minCountSeqs(seq, st, rl)
            assert host(mn).dtype.itemsize == bits // 8
            poison.assert_same("minimum counts, %s" % what, mn, exp_min.astype(wm.DTYPES[bits]))
            poison.assert_bitmap("valid bits of minCountSeqs, %s" % what, vb, valid, n)
    if nbytes >= 64:  # minimum counts on both sides of the thresholds 1 and 256
        assert min(seen) == 0 and any(0 < v < 256 for v in seen) and any(v >= 256 for v in seen)
    for f in filters:
        assert f.download().tobytes() == raw.tobytes()
        f.close()


# ---------------------------------------------------------------------------------------------------------------
# raw k-mers: hash rows with a row_valid byte
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kmers(oracle):
    """k-mers of 22 bases, each several times over, with k-mers that have no hash value among them -> (k, h, buffer, hash
    rows, valid flags).  NTC64 takes the bases four at a time through tables that give every byte some value, and checks
    the k % 4 bases that are left over: a k-mer is invalid when an N or a byte outside the alphabet is among its last two
    (an N further up is hashed like any base: such a k-mer is among the valid ones)"""
    k, h = 22, 3
    rng = np.random.RandomState(7)
    good = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for _ in range(40)]
    good.append(good[4][:7] + b"N" + good[4][8:])
    bad = [good[0][:-1] + b"N", good[1][:-2] + b"\x01" + good[1][-1:], good[2][:-1] + b"\xff", good[3][:-1] + b"-"]
    items = [s for s in good for _ in range(rng.randint(1, 41))] + [s for s in bad for _ in range(6)]
    items = [items[i] for i in rng.permutation(len(items))]
    buf = b"".join(items)
    hv, ok = oracle.kmer_hashes(buf, k, h)
    is_bad = np.array([s in bad for s in items])
    assert (ok.astype(bool) == ~is_bad).all() and is_bad.sum() == 24
    return k, h, buf, hv, ok.astype(bool)


@pytest.mark.parametrize("mem", ["host", "device+2"])
@pytest.mark.parametrize("nbytes", [64, 1000])
@pytest.mark.parametrize("bits", WIDTHS)
def test_raw_kmers_with_invalid_ones_among_them(eng, kmers, bits, nbytes, mem):
    k, h, buf, hv, ok = kmers
    mx = wm.max_of(bits)
    raw, before = body_of(bits, nbytes)
    a = np.frombuffer(buf, np.uint8).copy()
    seq = a if mem == "host" else device_slice(a, 2)
    thr = 256
    f = eng.CountingBloomFilter(nbytes, h, k, thr, counter_bits=bits)
    size = f.size()
    pos = uo.positions(hv[ok], size)  # the probes of the valid k-mers alone
    upper = wm.increment_all_exact(before, pos, mx)
    # contains: 0 for the invalid k-mers, the model's answer for the others (both occur)
    f.upload(raw)
    want = np.zeros(len(ok), np.uint8)
    want[ok] = before[pos].min(axis=1) >= np.uint64(thr)
    assert 0 < want[ok].sum() < ok.sum()
    poison.assert_same("containsKmers", f.containsKmers(seq), want)
    assert f.download().tobytes() == raw.tobytes()
    # serial order: the model's body, in which the invalid k-mers change nothing
    for op in ("min", "all"):
        model = wm.WideCBF(bits, nbytes, h, k, thr, raw.tobytes())
        for row in hv[ok]:
            (model.increment_min if op == "min" else model.increment_all)(row)
        f.upload(raw)
        f.insertKmers(seq, increment_all=op == "all", serial=True)
        poison.assert_same("insertKmers, serial, %s" % op, f.download(), np.frombuffer(model.body(), np.uint8))
    # parallel order: incrementAll exact, incrementMin by contract -- M1 names a counter that only an invalid k-mer's
    # (undefined) hash row could have reached
    f.upload(raw)
    f.insertKmers(seq, increment_all=True)
    wm.check_increment_all(f.counters(), upper)
    f.upload(raw)
    f.insertKmers(seq)
    wm.check_increment_min(before, f.counters(), upper, pos, mx)
    f.close()
