"""miBF (btlbf_mibf_*) checks that need no GPU: the symbols, the argument and file errors reported before any HIP
call, and the numpy model of tests/mibf_model.py on hand-worked cases."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import mibf_model as mm

NAMES = ["btlbf_mibf_create", "btlbf_mibf_destroy", "btlbf_mibf_size", "btlbf_mibf_bits", "btlbf_mibf_hash_num",
         "btlbf_mibf_kmer_size", "btlbf_mibf_set_scratch", "btlbf_mibf_insert_ids_seqs", "btlbf_mibf_saturate_seqs",
         "btlbf_mibf_query_seqs", "btlbf_mibf_stats", "btlbf_mibf_id_counts", "btlbf_mibf_download",
         "btlbf_mibf_upload", "btlbf_mibf_download_counts", "btlbf_mibf_store", "btlbf_mibf_load"]
FAKE = C.c_void_p(16)  # never dereferenced: every call below fails before it looks at the filter


def test_library_exports_every_mibf_symbol(lib):
    from btl_bloomfilter_amd import _lib

    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTS


def test_bad_id_bytes_is_einval(lib):
    m = C.c_void_p()
    for b in (0, 1, 3, 8):
        assert lib.btlbf_mibf_create(C.byref(m), FAKE, b) == 1
        assert b"id_bytes" in lib.btlbf_last_error()
        assert lib.btlbf_mibf_load(C.byref(m), b"/nonexistent.mibf", FAKE, b) == 1


def test_missing_file_is_eio(lib):
    m = C.c_void_p()
    assert lib.btlbf_mibf_load(C.byref(m), b"/nonexistent/x.mibf", FAKE, 2) == 3


@pytest.mark.parametrize("what", ["magic", "hlen", "version", "length", "short"])
def test_corrupt_files_are_eformat(lib, tmp_path, what):
    data = np.arange(10, dtype=np.uint16)
    seeds = ["1101", "1011"]
    raw = bytearray(mm.file_bytes(data, 2, 2, 4, seeds))
    if what == "magic":
        raw[0:8] = b"MIBLOOMX"
    elif what == "hlen":
        raw[8:12] = struct.pack("<I", 33)
    elif what == "version":
        raw[28:32] = struct.pack("<I", 2)
    elif what == "length":
        raw += b"\0\0"
    else:
        raw = raw[:-2]
    p = tmp_path / "x.mibf"
    p.write_bytes(bytes(raw))
    m = C.c_void_p()
    assert lib.btlbf_mibf_load(C.byref(m), str(p).encode(), FAKE, 2) == 4
    # the same body read as uint32 IDs has the wrong length
    p.write_bytes(mm.file_bytes(data, 2, 2, 4, seeds))
    assert lib.btlbf_mibf_load(C.byref(m), str(p).encode(), FAKE, 4) == 4


def test_model_header_is_the_packed_struct():
    """#pragma pack(1) FileHeader {char magic[8]; uint32 hlen; uint64 size; uint32 nhash, kmer, version} (MIBloomFilter.hpp:106-117)"""
    hd = mm.header(1234567, 4, 31, ["1" * 31] * 4)
    assert len(hd) == 32 + 4 * 31
    assert hd[:8] == b"MIBLOOMF"
    assert struct.unpack_from("<I", hd, 8)[0] == 32 + 4 * 31
    assert struct.unpack_from("<Q", hd, 12)[0] == 1234567
    assert struct.unpack_from("<III", hd, 20) == (4, 31, 1)
    assert mm.header(5, 3, 25)[8:12] == struct.pack("<I", 32)


class _R:
    """rank() of a bit vector with every bit set: rank(v) = v % size"""

    def __init__(self, size):
        self.size = size

    def rank(self, hv):
        return (np.asarray(hv, np.uint64) % np.uint64(self.size)).astype(np.int64)


def test_model_reservoir_by_hand():
    # one sequence, id 5, two distinct values at rank 0 (size 4): 4 and 8 (ascending), 4 twice (counted once)
    data, counts = np.zeros(4, np.int64), np.zeros(4, np.int64)
    rows = np.array([[8, 4], [4, 4]], np.uint64)
    mm.insert_ids(data, counts, _R(4), rows, np.array([True, True]), np.array([0, 0]), [5], 2)
    # v=4: c=1, x=(4^5)%1=0 == 0 -> data=5; v=8: c=2, x=(8^5)=13, 13%2=1 == 1 -> data=5
    assert counts.tolist() == [2, 0, 0, 0] and data.tolist() == [5, 0, 0, 0]
    # a second sequence, id 6, value 12 at rank 0: c=3, x=12^6=10, 10%3=1 != 2 -> no replacement
    mm.insert_ids(data, counts, _R(4), np.array([[12]], np.uint64), np.array([True]), np.array([0]), [6], 2)
    assert counts[0] == 3 and data[0] == 5
    # ... value 1 at rank 1 of a saturated entry: setData keeps the bit (old value > mask)
    data[1] = 0x8003
    mm.insert_ids(data, counts, _R(4), np.array([[1]], np.uint64), np.array([True]), np.array([0]), [7], 2)
    assert data[1] == 0x8007 and counts[1] == 1
    # old value == mask exactly is not "saturated" (strict >)
    data[2] = 0x8000
    mm.insert_ids(data, counts, _R(4), np.array([[2]], np.uint64), np.array([True]), np.array([0]), [7], 2)
    assert data[2] == 7


def test_model_counter_wrap():
    # uint16: a count of 0xffff wraps to 0 -> no replacement; the next arrival is c = 1 -> replacement
    data, counts = np.zeros(2, np.int64), np.array([0xffff, 0], np.int64)
    mm.insert_ids(data, counts, _R(2), np.array([[0], [2]], np.uint64), np.array([True, True]), np.array([0, 1]),
                  [3, 9], 2)
    assert counts[0] == 1 and data[0] == 9


def test_model_saturation_rules_by_hand():
    # h = 3, all three positions hold other ids: 4, 4, 6 -> 4 repeats, so positions 0 and 1 qualify; the larger
    # count wins (strict >, first maximum)
    data = np.array([4, 4, 6, 0], np.int64)
    counts = np.array([2, 5, 9, 0], np.int64)
    rows = np.array([[0, 1, 2]], np.uint64)
    d, c = data.copy(), counts.copy()
    out = mm.saturate_serial(d, c, _R(4), rows, np.array([True]), np.array([0]), [7], 2)
    assert out == [1, 0, 1, 0] and d.tolist() == [4, 7, 6, 0] and c.tolist() == [2, 6, 9, 0]
    # all distinct and nonzero: nothing qualifies -> saturate all three
    d = np.array([3, 4, 6, 0], np.int64)
    c = counts.copy()
    out = mm.saturate_serial(d, c, _R(4), rows, np.array([True]), np.array([0]), [7], 2)
    assert out == [1, 0, 0, 1] and d.tolist() == [0x8003, 0x8004, 0x8006, 0]
    # a zero entry with count 0 qualifies but loses to the start value 0 of the search -> saturate
    d = np.array([0, 4, 6, 0], np.int64)
    c = np.array([0, 1, 1, 0], np.int64)
    out = mm.saturate_serial(d, c, _R(4), rows, np.array([True]), np.array([0]), [7], 2)
    assert out[3] == 1
    # the id is found: nothing happens
    d = np.array([0x8007, 4, 6, 0], np.int64)
    out = mm.saturate_serial(d, counts.copy(), _R(4), rows, np.array([True]), np.array([0]), [7], 2)
    assert out == [1, 1, 0, 0] and d[0] == 0x8007
    # parallel: two windows choose position 1 against the same snapshot; the count rises by two, the last id wins
    data = np.array([4, 4, 6, 0], np.int64)
    d, c = data.copy(), counts.copy()
    out = mm.saturate_parallel(d, c, _R(4), np.array([[0, 1, 2], [0, 1, 2]], np.uint64), np.array([True, True]),
                               np.array([0, 1]), [7, 8], 2)
    assert out == [2, 0, 2, 0] and d[1] == 8 and c[1] == 7


def test_cpp_header_compiles_as_cpp11(tmp_path):
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "btlbf/MIBloomFilter.hpp"\ntemplate class btlbf::MIBloomFilter<uint16_t>;\n'
                   'template class btlbf::MIBloomFilter<uint32_t>;\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-fsyntax-only", "-I" + os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
