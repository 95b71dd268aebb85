"""The read screen (btlbf_screen_*) without a GPU: the symbols; every argument error that is reported before any HIP call,
with a handle that is never dereferenced and outputs untouched; the refusals that look at the filters, on the library's
own filter objects built on the host by tests/cpp/test_screen_refusals.cpp (a handle cannot be made without a GPU); the
host arithmetic of csrc/screen_plan.hpp against brute force under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/cpp/test_screen_plan.cpp, a stand-alone program); and the C++ layer compiling against the header."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

FAKE = 16  # never dereferenced: every call below fails before it looks at a filter
NEW = ["btlbf_screen_seqs", "btlbf_screen_tally", "btlbf_screen_fastx_open", "btlbf_screen_fastx_next",
       "btlbf_screen_fastx_tally", "btlbf_screen_fastx_close", "btlbf_screen_fastx"]
ptr = lambda a: C.c_void_p(a.ctypes.data)


def test_library_exports_the_symbols(lib):
    from btl_bloomfilter_amd import _lib

    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.SCREEN_MAX_FILTERS == 16 and C.sizeof(_lib.ScreenParams) == 16
    text = open(os.path.join(ROOT, "include", "btlbf.h")).read()
    assert "BTLBF_SCREEN_MAX_FILTERS = 16" in text
    import btl_bloomfilter_amd as m

    assert callable(m.screenSeqs) and callable(m.screen_tally) and callable(m.screenFile)


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def test_argument_errors_before_any_filter_is_looked_at(lib, tmp_path):
    from btl_bloomfilter_amd import _lib as L

    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    path = str(fq).encode()
    seq = np.frombuffer(b"ACGT" * 10, np.uint8).copy()
    outs = [np.full(32, 7, np.uint32), np.full(2, 7, np.uint32), np.full(2, 7, np.uint32)]
    tot = [np.full(16, 7, np.uint64), np.full(16, 7, np.uint64), np.full(4, 7, np.uint64)]

    def both(fs, n, par, word):
        """screen_seqs, screen_fastx_open and screen_fastx refuse alike"""
        p = C.byref(par) if par is not None else None
        assert lib.btlbf_screen_seqs(fs, n, ptr(seq), 40, None, p, *[ptr(o) for o in outs], L.HOST, None) == L.EINVAL
        assert word in lib.btlbf_last_error(), lib.btlbf_last_error()
        h = C.c_void_p(99)
        assert lib.btlbf_screen_fastx_open(C.byref(h), fs, n, path, 0, p, 0) == L.EINVAL and not h.value
        assert word in lib.btlbf_last_error(), lib.btlbf_last_error()
        assert lib.btlbf_screen_fastx(fs, n, path, 0, p, 0, *[ptr(t) for t in tot], None) == L.EINVAL
        assert all((o == 7).all() for o in outs) and all((t == 7).all() for t in tot)

    ok = L.ScreenParams(0.5, 1, 0)
    two = handles(FAKE, FAKE + 16)
    both(None, 2, ok, b"null")
    both(two, 2, None, b"null")
    both(two, 0, ok, b"n_filters")
    both(handles(*range(FAKE, FAKE + 17 * 16, 16)), 17, ok, b"n_filters")
    both(handles(FAKE, None, FAKE + 16), 3, ok, b"null handle")
    both(handles(FAKE, FAKE + 16, FAKE + 32, FAKE + 16), 4, ok, b"twice")
    for bad in (-0.5, 1.5, float("nan"), float("inf")):
        both(two, 2, L.ScreenParams(bad, 1, 0), b"min_fraction")
    # the in-memory call's own: outputs, the buffer, the memory space, a length that is no multiple of read_len
    for null in (6, 7):
        args = [two, 2, ptr(seq), 40, None, C.byref(ok)] + [ptr(o) for o in outs] + [L.HOST, None]
        args[null] = None
        assert lib.btlbf_screen_seqs(*args) == L.EINVAL and b"null" in lib.btlbf_last_error()
    assert lib.btlbf_screen_seqs(two, 2, None, 40, None, C.byref(ok), *[ptr(o) for o in outs], L.HOST, None) == L.EINVAL
    assert lib.btlbf_screen_seqs(two, 2, ptr(seq), 40, None, C.byref(ok), *[ptr(o) for o in outs], 5, None) == L.EINVAL
    lay = L.Layout(None, 0, 30)
    assert lib.btlbf_screen_seqs(two, 2, ptr(seq), 40, C.byref(lay), C.byref(ok), *[ptr(o) for o in outs], L.HOST, None) == L.EINVAL
    assert b"read_len" in lib.btlbf_last_error() and all((o == 7).all() for o in outs)
    # the file handle's own
    h = C.c_void_p(99)
    assert lib.btlbf_screen_fastx_open(None, two, 2, path, 0, C.byref(ok), 0) == L.EINVAL
    assert lib.btlbf_screen_fastx_open(C.byref(h), two, 2, None, 0, C.byref(ok), 0) == L.EINVAL
    missing = str(tmp_path / "missing.fq").encode()
    assert lib.btlbf_screen_fastx_open(C.byref(h), two, 2, missing, 0, C.byref(ok), 0) == L.EIO and not h.value
    assert b"missing.fq" in lib.btlbf_last_error()
    n = C.c_uint64(7)
    assert lib.btlbf_screen_fastx_next(None, C.byref(n), C.byref(n), None, None, None) == L.EINVAL
    assert lib.btlbf_screen_fastx_tally(None, *[ptr(t) for t in tot]) == L.EINVAL
    lib.btlbf_screen_fastx_close(None)
    for i in range(3):  # the whole-file call's own outputs
        args = [two, 2, path, 0, C.byref(ok), 0] + [ptr(t) for t in tot] + [None]
        args[6 + i] = None
        assert lib.btlbf_screen_fastx(*args) == L.EINVAL
    assert all((t == 7).all() for t in tot)


def test_tally_argument_errors(lib):
    from btl_bloomfilter_amd import _lib as L

    hits, valid, pb = np.zeros((2, 3), np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    tot = [np.full(3, 7, np.uint64), np.full(3, 7, np.uint64), np.full(4, 7, np.uint64)]

    def tally(null=None, nf=3, mem=L.HOST):
        args = [ptr(hits), ptr(valid), ptr(pb), 2, nf] + [ptr(t) for t in tot] + [mem, 0, None]
        if null is not None:
            args[null] = None
        rc = lib.btlbf_screen_tally(*args)
        assert all((t == 7).all() for t in tot)
        return rc

    for null in (0, 1, 2, 5, 6, 7):
        assert tally(null=null) == L.EINVAL and b"null" in lib.btlbf_last_error(), null
    assert tally(nf=0) == L.EINVAL and tally(nf=17) == L.EINVAL and b"n_filters" in lib.btlbf_last_error()
    assert tally(mem=9) == L.EINVAL


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_refusals_on_filter_objects(tmp_path):
    exe = str(tmp_path / "test_screen_refusals")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function",
                        os.path.join(ROOT, "tests", "cpp", "test_screen_refusals.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    r = subprocess.run([exe, str(fq)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all screen refusals in place" in r.stdout, r.stdout + r.stderr


def test_screen_plan_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_screen_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           os.path.join(ROOT, "tests", "cpp", "test_screen_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "screen plan test passed" in r.stdout


def test_cpp_layer_compiles_on_cpu(tmp_path):
    from test_gpu_cpp_screen import build_program

    assert os.path.exists(build_program(tmp_path, os.path.join("examples", "bloom_screen.cpp")))
    assert os.path.exists(build_program(tmp_path, os.path.join("tests", "cpp", "test_screen_shim.cpp")))
