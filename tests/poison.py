"""Dirty output buffers with guard bands, for tests of the C ABI's output contract (include/btlbf.h: the caller need not
initialise an output, and nothing outside [out, out + size) is written).

The engine hands the library a zeroed buffer for every output (engine._out), so a byte that a call never stores reads
back as the zero the engine put there, and a store past an output lands in some other allocation.  Here every output is
carved out of a larger uint8 allocation of GUARD + nbytes + GUARD bytes, all set to one poison byte:

    poisoned_outputs(monkeypatch, byte)   engine._out replaced for the test; returns the Poison registry
    Poison.alloc(shape, dtype, ...)       one such output for a raw ctypes call -> (output, c_void_p)
    check_guards()                        every guard byte of every allocation of the active registry still is the poison

and the expectation side builds WHOLE outputs -- full_bitmap: ceil(n / 64) words with the positions >= n zero -- so
that a comparison covers every byte (assert_same), not the valid rows or bits alone.  A test runs under two poisons
(POISONS): an unwritten byte whose right value happens to be one of them is caught by the other."""
import ctypes as C
import sys

import numpy as np

GUARD = 256  # bytes before and after a payload: keeps the payload at the alignment of the allocation itself
POISONS = (0xFF, 0xA5)

_active = None  # the registry of the running test (poisoned_outputs sets it, monkeypatch's undo clears it)


def _torch_dtype(dtype):
    import torch

    name = np.dtype(dtype).name
    return getattr(torch, name if name == "uint8" else name.lstrip("u"))  # (as engine._out: torch's signed twin)


class Poison:
    """the allocations of one test: (name, whole uint8 allocation, payload bytes)"""

    def __init__(self, byte):
        self.byte = int(byte)
        self.allocs = []

    def alloc(self, shape, dtype, device=None, name=None):
        """an output of `shape` and `dtype` inside GUARD + nbytes + GUARD poisoned bytes -> (output, its c_void_p).
        device: a torch device (the output is a torch tensor there) or None (numpy, host memory)"""
        shape = shape if isinstance(shape, tuple) else (int(shape),)
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        name = "%s %s%s" % (name or "#%d" % len(self.allocs), dt.name, list(shape))
        if device is not None:
            import torch

            raw = torch.full((GUARD + nbytes + GUARD,), self.byte, dtype=torch.uint8, device=device)
            out = raw[GUARD:GUARD + nbytes].view(_torch_dtype(dt)).view(shape)
            ptr = raw.data_ptr() + GUARD
        else:
            raw = np.full(GUARD + nbytes + GUARD, self.byte, np.uint8)
            out = raw[GUARD:GUARD + nbytes].view(dt).reshape(shape)
            ptr = raw.ctypes.data + GUARD
        self.allocs.append((name, raw, nbytes))
        return out, C.c_void_p(ptr)

    def check_guards(self):
        """after the device has finished: every guard byte of every allocation still holds the poison"""
        if any(not isinstance(raw, np.ndarray) for _, raw, _ in self.allocs):
            import torch

            torch.cuda.synchronize()
        for name, raw, nbytes in self.allocs:
            host = raw if isinstance(raw, np.ndarray) else raw.cpu().numpy()
            for side, lo in (("leading", 0), ("trailing", GUARD + nbytes)):
                bad = np.flatnonzero(host[lo:lo + GUARD] != self.byte)
                if bad.size:
                    off = int(bad[0]) - GUARD if side == "leading" else nbytes + int(bad[0])
                    raise AssertionError("%s: %s guard overwritten: %d byte(s), the first at offset %d of the output "
                                         "(0x%02x, poison 0x%02x)" % (name, side, bad.size, off, host[lo + bad[0]], self.byte))


def poisoned_outputs(monkeypatch, byte):
    """engine._out for the rest of the test: the same (output, c_void_p) shapes and dtypes in the memory space of the
    input, but poisoned and guarded instead of zeroed.  Returns the registry."""
    from btl_bloomfilter_amd import engine

    global _active
    reg = Poison(byte)

    def _out(b, shape, dtype):
        if shape is None:
            return None, None
        shape = shape if isinstance(shape, tuple) else (int(shape),)
        caller = sys._getframe(1).f_code.co_name
        name = "%s#%d" % (caller, len(reg.allocs))
        if b.mem == engine.DEVICE:
            return reg.alloc(shape, dtype, device=b.keep.device, name=name)
        # (as engine._out: at least one element along the first axis, sliced back to the shape asked for)
        a, ptr = reg.alloc((max(shape[0], 1),) + shape[1:], dtype, name=name)
        return a[: shape[0]], ptr

    monkeypatch.setattr(engine, "_out", _out)
    monkeypatch.setattr(sys.modules[__name__], "_active", reg)
    return reg


def check_guards():
    assert _active is not None, "check_guards() outside poisoned_outputs()"
    assert _active.allocs, "no output was allocated under poison"
    _active.check_guards()


def host_bytes(x):
    """every byte of an output (numpy array or torch tensor) as a flat uint8 numpy array"""
    if not isinstance(x, np.ndarray):
        x = x.contiguous().cpu().numpy()
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def assert_same(name, got, want):
    """every byte of the output `got` equals the expectation `want` (same byte length); names the first difference"""
    g, w = host_bytes(got), host_bytes(np.asarray(want))
    assert g.size == w.size, "%s: %d bytes, expected %d" % (name, g.size, w.size)
    bad = np.flatnonzero(g != w)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d bytes differ, the first at byte %d: 0x%02x, expected 0x%02x"
                             % (name, bad.size, g.size, i, g[i], w[i]))


def full_bitmap(bits_bool, n):
    """the whole per-window bitmap of a buffer of n bytes from a boolean per window: ceil(n / 64) uint64 words, bit
    p & 63 of word p >> 6 for window p, the positions >= n zero"""
    b = np.asarray(bits_bool).astype(bool).ravel()
    assert b.size <= n or not b[n:].any(), "expectation has a window at or beyond n"
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[: min(b.size, n)] = b[:n]
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def assert_bitmap(name, got_words, bits_bool, n):
    """a bitmap output against full_bitmap, word for word; a set bit at a position >= n is named as such"""
    want = full_bitmap(bits_bool, n)
    g = host_bytes(got_words)
    assert g.size == want.size * 8, "%s: %d bytes, expected %d words" % (name, g.size, want.size)
    got_bits = np.unpackbits(g, bitorder="little")
    want_bits = np.unpackbits(want.view(np.uint8), bitorder="little")
    bad = np.flatnonzero(got_bits != want_bits)
    if bad.size:
        p = int(bad[0])
        where = "beyond the buffer's %d windows (tail of the last word)" % n if p >= n else "window %d" % p
        raise AssertionError("%s: %d bits differ, the first at position %d, %s: %d, expected %d"
                             % (name, bad.size, p, where, got_bits[p], want_bits[p]))


def full_rows(n, width, dtype, pos, rows):
    """[n, width] array of `dtype`, zero except rows `pos`"""
    out = np.zeros((n, width), dtype)
    if len(pos):
        out[np.asarray(pos, np.int64)] = rows
    return out
