"""The edges of the wide-counter kernels' grids (csrc/wide_counter_kernels.hip), which no other test reaches:
  * wide_seq_kernel with more than one tile per workgroup (its `for t` loop with tile_off stepping): more than 8 * CUs
    tiles -- some 8.4 MB on 256 CUs;
  * wide_rows_kernel on a second trip of its grid-stride loop: more than 2048 * 256 rows;
  * wide_popcount_kernel and wide_compare_kernel on a second trip: more than 4096 * 256 * 16 bytes = 16 MiB of counters.
Everything is integer-exact or one of the contract inequalities M1-M4 of tests/wide_counter_model.py.  The sequence test
computes its expectation from ONE read's hash rows times the number of copies: no per-window array of hash rows is built."""
import numpy as np
import pytest

import poison
import update_order_model as uo
import wide_counter_model as wm
import wide_update_order_model as w

pytestmark = pytest.mark.gpu
WIDTHS = (16, 32, 64)
HASHING = {"h3": (31, 3), "h5": (25, 5)}  # h <= 4: the pipelined query; h = 5: the plain loop
READ_LEN = 4099  # longer than a tile, and 2048 is no multiple of it: every tile begins at another offset of the read


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.zeros(1, device="cuda")
    from btl_bloomfilter_amd import engine

    return engine


def body_of(bits, nbytes):
    n = wm.round_bytes(nbytes) * 8 // bits
    raw = wm.prefilled_body(bits, n, 11)
    return np.frombuffer(raw, np.uint8), np.frombuffer(raw, wm.DTYPES[bits]).astype(np.uint64)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def device(a):
    import torch

    a = np.array(a)  # (a writable copy: torch takes no read-only arrays)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


# ---------------------------------------------------------------------------------------------------------------
# more than one tile per workgroup
# ---------------------------------------------------------------------------------------------------------------
def launch_geometry(n_bytes, cus):
    """launch_wide_seq_op's arithmetic -> (tiles, tiles per workgroup, workgroups)"""
    n_tiles = (n_bytes + w.TILE - 1) // w.TILE
    blocks = min(n_tiles, 8 * cus)
    per_block = (n_tiles + blocks - 1) // blocks
    return n_tiles, per_block, (n_tiles + per_block - 1) // per_block


@pytest.fixture(scope="module")
def long_buffer(oracle):
    """copies of one 4099-base read with a few unclean bytes, (16 * CUs + 5) tiles and a few bytes in all.  The C ABI
    takes a uniform layout only for whole reads (EINVAL otherwise), so the buffer comes in two forms:
      partial = False  whole copies, to go under read_len = 4099 (tile_off stepping);
      partial = True   34 bytes of one more copy behind them -- 37 bytes into the last tile -- under explicit starts.
    -> get(hashing, partial) = (device tensor, layout keywords, bytes, copies, (window offsets, hash rows) of the read,
    the same of the partial last read)"""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_all = (16 * cus + 5) * w.TILE + 37
    copies, tail = divmod(n_all, READ_LEN)
    rng = np.random.RandomState(4099)
    read = uo._dirty(rng, uo._acgt(rng, READ_LEN), 0.001, at_least_one=True)
    whole = np.frombuffer(read * copies + read[:tail], np.uint8).copy()
    dev = device(whole)
    for n in (n_all, copies * READ_LEN):  # both forms: several tiles per workgroup and a short last workgroup
        n_tiles, per_block, blocks = launch_geometry(n, cus)
        assert per_block >= 2 and n_tiles > 8 * cus and n_tiles % per_block, (cus, n, n_tiles, per_block)
    starts = device(np.append(np.arange(0, n_all, READ_LEN), n_all).astype(np.uint64))
    cache = {}

    def get(hashing, partial=False):
        if hashing not in cache:
            k, h = HASHING[hashing]
            c1, hv1 = oracle.nthash_seq(read, h, k)
            c2, hv2 = oracle.nthash_seq(read[:tail], h, k)
            assert 0 < READ_LEN - k + 1 - len(c1) < 400, len(c1)  # a few unclean bytes, most windows clean
            cache[hashing] = (c1.astype(np.int64), hv1), (c2.astype(np.int64), hv2.reshape(-1, h))
        one, last = cache[hashing]
        if partial:
            assert tail and len(starts) == copies + 2
            return dev, {"starts": starts}, n_all, copies, one, last
        none = (np.zeros(0, np.int64), np.zeros((0, HASHING[hashing][1]), np.uint64))
        return dev[: copies * READ_LEN], {"read_len": READ_LEN}, copies * READ_LEN, copies, one, none

    return get


def spread(n, copies, c1, v1, c2, v2, dtype):
    """a per-window value of the read's clean windows (v1 at offsets c1) and of the tail's, laid over the whole buffer"""
    one = np.zeros(READ_LEN, dtype)
    one[c1] = v1
    last = np.zeros(n - copies * READ_LEN, dtype)
    last[c2] = v2
    return np.concatenate([np.tile(one, copies), last])


def check_queries(f, bits, thr, dev, lay, n, copies, c1, pos1, c2, pos2, state, what):
    m1 = state[pos1].min(axis=1)
    m2 = state[pos2].min(axis=1) if len(pos2) else np.zeros(0, np.uint64)
    exp_min = spread(n, copies, c1, m1, c2, m2, np.uint64)
    valid = spread(n, copies, c1, True, c2, True, bool)
    exp_hit = valid & (exp_min >= np.uint64(thr))
    assert 0 < exp_hit.sum() and (what != "before" or exp_hit.sum() < valid.sum())
    hit, vb, cnt = f.containsSeqs(dev, want_counts=True, **lay)
    poison.assert_bitmap("hit bits, " + what, hit, exp_hit, n)
    poison.assert_bitmap("valid bits, " + what, vb, valid, n)
    assert host(cnt).view(np.uint64).tolist() == [int(valid.sum()), int(exp_hit.sum())], what
    mn, vb = f.minCountSeqs(dev, **lay)
    poison.assert_same("minimum counts, " + what, mn, exp_min.astype(wm.DTYPES[bits]))
    poison.assert_bitmap("valid bits of minCountSeqs, " + what, vb, valid, n)


@pytest.mark.parametrize("hashing", list(HASHING))
@pytest.mark.parametrize("bits", WIDTHS)
def test_several_tiles_per_workgroup_increment_all_and_queries(eng, long_buffer, bits, hashing):
    k, h = HASHING[hashing]
    mx = wm.max_of(bits)
    dev, lay, n, copies, (c1, hv1), (c2, hv2) = long_buffer(hashing)
    raw, before = body_of(bits, 1000)
    f = eng.CountingBloomFilter(1000, h, k, 256, counter_bits=bits)
    size = f.size()
    pos1, pos2 = uo.positions(hv1, size), uo.positions(hv2, size)
    add = copies * np.bincount(pos1.ravel(), minlength=size) + np.bincount(pos2.ravel(), minlength=size)
    upper = wm.saturating_add(before, add, mx)
    if bits == 16:  # saturation from the call's own increments
        assert ((before <= 0x100) & (upper == mx)).any() and (upper[add > 0] < mx).any()
    f.upload(raw)
    check_queries(f, bits, 256, dev, lay, n, copies, c1, pos1, c2, pos2, before, "before")
    f.insertSeqs(dev, increment_all=True, **lay)
    after = f.counters().astype(np.uint64)
    wm.check_increment_all(after, upper)
    check_queries(f, bits, 256, dev, lay, n, copies, c1, pos1, c2, pos2, upper, "after incrementAll")
    f.close()


def test_several_tiles_per_workgroup_under_starts_with_a_partial_last_read(eng, long_buffer):
    bits, (k, h) = 16, HASHING["h3"]
    mx = wm.max_of(bits)
    dev, lay, n, copies, (c1, hv1), (c2, hv2) = long_buffer("h3", partial=True)
    assert len(c2) > 0
    raw, before = body_of(bits, 4096)
    f = eng.CountingBloomFilter(4096, h, k, 256, counter_bits=bits)
    size = f.size()
    pos1, pos2 = uo.positions(hv1, size), uo.positions(hv2, size)
    add = copies * np.bincount(pos1.ravel(), minlength=size) + np.bincount(pos2.ravel(), minlength=size)
    upper = wm.saturating_add(before, add, mx)
    # M1-M3 are statements about counters and about DISTINCT windows: the read's and the tail's windows stand for all
    # their copies.  M4 counts windows, and is off whenever a probed counter can reach the maximum -- as here
    pos = np.concatenate([pos1, pos2])
    assert int(upper[np.unique(pos)].max()) == mx
    f.upload(raw)
    f.insertSeqs(dev, **lay)
    wm.check_increment_min(before, f.counters(), upper, pos, mx)
    f.upload(raw)
    f.insertSeqs(dev, increment_all=True, **lay)
    wm.check_increment_all(f.counters(), upper)
    check_queries(f, bits, 256, dev, lay, n, copies, c1, pos1, c2, pos2, upper, "after incrementAll")
    f.close()


# ---------------------------------------------------------------------------------------------------------------
# hash rows: the second trip of wide_rows_kernel's grid-stride loop
# ---------------------------------------------------------------------------------------------------------------
N_ROWS = 2048 * 256 + 1000


@pytest.fixture(scope="module")
def many_rows(oracle):
    """the rows of the 1000-byte case's reads, tiled and shuffled to N_ROWS"""
    nbytes, h, k, thr, reads, _ = wm.make_case("c1000", 16)
    _, rows = uo.clean_windows(oracle, b"".join(reads), k, h, starts=np.cumsum([0] + [len(s) for s in reads]))
    c = N_ROWS // len(rows) + 1
    big = np.ascontiguousarray(uo.duplicated_rows(5, rows, c, c)[:N_ROWS])
    assert big.shape == (N_ROWS, h) and N_ROWS > 2048 * 256
    assert len(np.unique(big[2048 * 256:], axis=0)) > 50  # the second trip holds many different rows
    return nbytes, h, k, big


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("bits", [16, 64])
def test_min_count_of_more_rows_than_the_grid_has_lanes(eng, many_rows, bits, mem):
    nbytes, h, k, big = many_rows
    raw, before = body_of(bits, nbytes)
    f = eng.CountingBloomFilter(nbytes, h, k, 256, counter_bits=bits)
    f.upload(raw)
    exp = before[uo.positions(big, f.size())].min(axis=1)
    assert (exp > 255).any() and (exp < 256).any() and len(set(exp[2048 * 256:].tolist())) > 2
    rows = big if mem == "host" else device(big)
    poison.assert_same("minCount", f.minCount(rows), exp.astype(wm.DTYPES[bits]))
    poison.assert_same("contains", f.contains(rows), (exp >= 256).astype(np.uint8))
    f.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_updates_of_more_rows_than_the_grid_has_lanes(eng, many_rows, bits):
    nbytes, h, k, big = many_rows
    mx = wm.max_of(bits)
    raw, before = body_of(bits, nbytes)
    f = eng.CountingBloomFilter(nbytes, h, k, 1, counter_bits=bits)
    pos = uo.positions(big, f.size())
    upper = wm.increment_all_exact(before, pos, mx)
    rows = device(big)
    f.upload(raw)
    f.incrementAll(rows)
    wm.check_increment_all(f.counters(), upper)
    f.upload(raw)
    f.insert(rows)
    wm.check_increment_min(before, f.counters(), upper, pos, mx)
    f.close()


# ---------------------------------------------------------------------------------------------------------------
# reductions: the second trip of the popcount and compare kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", WIDTHS)
def test_reductions_beyond_one_trip_of_the_grid(eng, bits):
    nbytes = (16 << 20) + 4096 + 8  # no multiple of 16: the zero padding of the last vector is not counted
    assert nbytes > 4096 * 256 * 16 and nbytes % 16 == 8
    n = nbytes * 8 // bits
    rng = np.random.RandomState(bits)
    vals = np.array(wm.prefill_values(bits) + (2, 300), dtype=np.uint64)
    a = vals[rng.randint(0, len(vals), n)].astype(wm.DTYPES[bits])
    b = a.copy()
    idx = rng.permutation(n)[: n // 3]
    b[idx] = vals[rng.randint(0, len(vals), len(idx))].astype(wm.DTYPES[bits])
    first = 4096 * 256 * 16 * 8 // bits  # counters of the first trip
    assert (a[first:] != b[first:]).any() and (a[first:] != 0).any()
    fb = eng.CountingBloomFilter(nbytes, 2, 8, 1, counter_bits=bits)
    fb.upload(b.view(np.uint8))
    for thr in (0, 1, 256, 0xffffffff):
        fa = eng.CountingBloomFilter(nbytes, 2, 8, thr, counter_bits=bits)
        assert fa.size() == n and fa.sizeInBytes() == nbytes
        fa.upload(a.view(np.uint8))
        assert fa.popCount() == int((a != 0).sum())
        assert fa.filtered_popcount() == int((a.astype(np.uint64) >= np.uint64(thr)).sum())
        if thr == 256:
            assert fa.compare(fb) == (int((a != b).sum()), int((a > b).sum()), int((a < b).sum()))
            assert fb.compare(fa) == (int((a != b).sum()), int((a < b).sum()), int((a > b).sum()))
            assert fa.digest() == eng.body_digest(a.view(np.uint8)) and fb.digest() == eng.body_digest(b.view(np.uint8))
        fa.close()
    fb.close()
