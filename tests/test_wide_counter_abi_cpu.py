"""The C ABI of the wide counting kinds (BTLBF_COUNTING16 / 32 / 64) without a GPU: the symbols, and every refusal that
is reported before any HIP call -- an unknown kind, btlbf_create_shard, a load whose header does not fit the width, a wide
file loaded as 8-bit counters; and, on the library's own filter object built on the host by
tests/cpp/test_wide_refusals.cpp (a handle cannot be made without a GPU): an explicit PARTITIONED mode, the byte forms
of the minimum counts with nothing written, shards, positions, routing, the micro-benchmark.  Last, the C++ shim
CountingBloomFilter<T> instantiated whole for the three wide T and linked against the stub ABI."""
import ctypes as C
import os
import subprocess

import pytest
from conftest import GOLDEN, ROOT

import wide_counter_model as wm

EINVAL, EFORMAT, EHIP = 1, 4, 5


def test_new_symbols_and_kinds(lib):
    from btl_bloomfilter_amd import _lib

    for name in ("btlbf_counter_bytes", "btlbf_min_count_seqs_wide", "btlbf_min_count_hashes_wide"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert (_lib.COUNTING16, _lib.COUNTING32, _lib.COUNTING64) == (2, 3, 4)
    assert _lib.COUNTING_KIND == wm.KINDS
    text = open(os.path.join(ROOT, "include", "btlbf.h")).read()
    assert "BTLBF_COUNTING16 = 2, BTLBF_COUNTING32 = 3, BTLBF_COUNTING64 = 4" in text


@pytest.mark.parametrize("kind", [2, 3, 4])
def test_wide_kinds_are_known_and_others_are_not(lib, kind):
    h = C.c_void_p()
    rc = lib.btlbf_create(C.byref(h), kind, 1000, 3, 25, 1, 0)
    if lib.btlbf_device_count() == 0:
        assert rc == EHIP and b"no CPU path" in lib.btlbf_last_error()  # (not "unknown filter kind")
    else:
        assert rc == 0 and lib.btlbf_kind(h) == kind and lib.btlbf_counter_bytes(h) == 1 << (kind - 1)
        assert lib.btlbf_size_bytes(h) == 1000 and lib.btlbf_size(h) * (1 << (kind - 1)) == 1000
        lib.btlbf_destroy(h)
    for bad in (5, 7, -1):
        assert lib.btlbf_create(C.byref(h), bad, 1000, 3, 25, 1, 0) == EINVAL
        assert b"unknown filter kind" in lib.btlbf_last_error()
        assert lib.btlbf_load(C.byref(h), bad, b"/nonexistent/x.bf", 1, 0) == EINVAL
        assert b"unknown filter kind" in lib.btlbf_last_error()
        assert lib.btlbf_create_from_header(C.byref(h), bad, b"x", 1, 1, 0) == EINVAL
    # no shards of a wide filter
    assert lib.btlbf_create_shard(C.byref(h), kind, 1 << 20, 0, 2, 3, 25, 1, 0) == EINVAL
    assert b"direct path only" in lib.btlbf_last_error() and not h.value


@pytest.mark.parametrize("bits", [16, 32, 64])
def test_load_checks_the_sizes_against_the_width(lib, bits):
    """before any HIP call: the errors come on a machine without a GPU, where a load that fits answers EHIP"""
    path = os.path.join(GOLDEN, wm.fixture_name("c1000", bits, "all")).encode()
    data = open(path, "rb").read()
    cut = data.index(b"[HeaderEnd]\n") + 12
    counters, nbytes = 1000 * 8 // bits, 1000
    h = C.c_void_p()
    for other in (8, 16, 32, 64):
        for call in (lambda k: lib.btlbf_load(C.byref(h), k, path, 1, 0),
                     lambda k: lib.btlbf_create_from_header(C.byref(h), k, data[:cut], cut, 1, 0)):
            rc = call(wm.KINDS[other])
            msg = lib.btlbf_last_error().decode()
            if other == bits:
                assert rc == (EHIP if lib.btlbf_device_count() == 0 else 0), msg
                if rc == 0:
                    lib.btlbf_destroy(h)
            elif other == 8:
                assert rc == EFORMAT and "only 8-bit counters are supported" in msg
            else:
                assert rc == EFORMAT and str(counters) in msg and str(nbytes) in msg and "%d-bit" % other in msg


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_refusals_on_a_wide_filter_object(tmp_path):
    exe = str(tmp_path / "test_wide_refusals")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function",
                        os.path.join(ROOT, "tests", "cpp", "test_wide_refusals.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all wide refusals in place" in r.stdout, r.stdout + r.stderr


def test_wide_shim_compiles_and_links_against_the_stub_abi(tmp_path):
    exe = str(tmp_path / "test_wide_shim_link")
    cpp = os.path.join(ROOT, "tests", "cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(cpp, "test_wide_shim_link.cpp"), os.path.join(cpp, "stub_abi.cpp"),
                        os.path.join(cpp, "stub_abi_wide.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "wide shim links" in r.stdout, r.stdout + r.stderr
