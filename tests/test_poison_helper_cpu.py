"""tests/poison.py can fail: with a "library call" written in numpy, each of the four things it exists to catch makes it
raise -- an unwritten payload byte, a write into the leading guard, one into the trailing guard, a tail bit set beyond
n -- and a call that does everything right passes.  No GPU: the host branch of the poisoned engine._out."""
import ctypes as C

import numpy as np
import pytest

import poison
from btl_bloomfilter_amd import engine

N = 100  # windows: two bitmap words, 28 tail positions in the last one
CLEAN = np.arange(N) % 3 != 0


def raw_bytes(ptr, lo, hi):
    """bytes [lo, hi) relative to an output's pointer, as the callee sees its memory"""
    return np.ctypeslib.as_array(C.cast(ptr.value + lo, C.POINTER(C.c_uint8)), shape=(hi - lo,))


def fake_call(p_valid, p_min, flaw=None):
    """what a correct library call does with a valid bitmap of N windows and N bytes of minimum counts; `flaw` breaks it"""
    words = poison.full_bitmap(CLEAN, N)
    if flaw == "tail bit":
        words[-1] |= np.uint64(1) << np.uint64(N % 64 + 5)
    raw_bytes(p_valid, 0, 16)[:] = words.view(np.uint8)
    mn = np.where(CLEAN, 7, 0).astype(np.uint8)
    raw_bytes(p_min, 0, N)[:] = mn
    if flaw == "unwritten":
        raw_bytes(p_min, 0, N)[41] = poison._active.byte  # as if the store had never happened
    if flaw == "leading guard":
        raw_bytes(p_min, -1, 0)[:] = 0
    if flaw == "trailing guard":
        raw_bytes(p_valid, 16, 24)[:] = 0  # one word past the bitmap


def run(monkeypatch, byte, flaw):
    poison.poisoned_outputs(monkeypatch, byte)
    b = engine._Buf(np.zeros(N, np.uint8))
    valid, p_valid = engine._out(b, engine._words(N), np.uint64)
    mn, p_min = engine._out(b, N, np.uint8)
    assert valid.shape == (2,) and valid.dtype == np.uint64 and mn.shape == (N,) and mn.dtype == np.uint8
    assert p_valid.value == valid.ctypes.data and p_min.value == mn.ctypes.data and p_min.value % 16 == p_valid.value % 16 == 0
    assert (poison.host_bytes(valid) == byte).all() and (poison.host_bytes(mn) == byte).all()  # dirty when handed out
    assert engine._out(b, None, np.uint64) == (None, None)
    fake_call(p_valid, p_min, flaw)
    poison.assert_bitmap("valid", valid, CLEAN, N)
    poison.assert_same("min", mn, np.where(CLEAN, 7, 0).astype(np.uint8))
    poison.check_guards()


@pytest.mark.parametrize("byte", poison.POISONS)
def test_a_correct_call_passes(monkeypatch, byte):
    run(monkeypatch, byte, None)


@pytest.mark.parametrize("byte", poison.POISONS)
@pytest.mark.parametrize("flaw,message", [
    ("unwritten", r"min: 1 of 100 bytes differ, the first at byte 41"),
    ("leading guard", r"uint8\[100\]: leading guard overwritten: 1 byte\(s\), the first at offset -1 "),
    ("trailing guard", r"uint64\[2\]: trailing guard overwritten: 8 byte\(s\), the first at offset 16 "),
    ("tail bit", r"valid: 1 bits differ, the first at position 105, beyond the buffer's 100 windows"),
])
def test_each_flaw_is_flagged(monkeypatch, byte, flaw, message):
    with pytest.raises(AssertionError, match=message):
        run(monkeypatch, byte, flaw)


def test_zero_length_first_axis_keeps_the_engines_shape(monkeypatch):
    """engine._out gives a host output at least one element along its first axis and slices it back"""
    poison.poisoned_outputs(monkeypatch, 0xA5)
    out, ptr = engine._out(engine._Buf(np.zeros(0, np.uint8)), (0, 4), np.uint64)
    assert out.shape == (0, 4) and ptr.value
    poison.check_guards()


def test_the_engine_itself_keeps_zeroing(monkeypatch):
    out, _ = engine._out(engine._Buf(np.zeros(8, np.uint8)), 8, np.uint8)
    assert not out.any()
    poison.poisoned_outputs(monkeypatch, 0xFF)
    monkeypatch.undo()
    out, _ = engine._out(engine._Buf(np.zeros(8, np.uint8)), 8, np.uint8)
    assert not out.any() and poison._active is None


def test_full_bitmap_whole_words():
    w = poison.full_bitmap(np.ones(65, bool), 65)
    assert w.dtype == np.uint64 and w.tolist() == [2**64 - 1, 1]
    assert poison.full_bitmap(np.ones(64, bool), 64).tolist() == [2**64 - 1]
    assert poison.full_bitmap(np.zeros(0, bool), 1).tolist() == [0]
    with pytest.raises(AssertionError):
        poison.full_bitmap(np.ones(66, bool), 65)
    rows = poison.full_rows(5, 2, np.uint64, [1, 3], np.array([[1, 2], [3, 4]], np.uint64))
    assert rows.tolist() == [[0, 0], [1, 2], [0, 0], [3, 4], [0, 0]]
