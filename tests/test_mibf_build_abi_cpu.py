"""The C ABI of the miBF builder without a GPU: the symbols and structures of btlbf_mibf_build_fastx,
btlbf_mibf_optimal_size and the window counters, and every entry check -- tests/cpp/test_mibf_build_refusals.cpp calls
them with a device that does not exist, so that a call which passes the checks says "no GPU" and a refused one its own
code first: the checks come before any HIP call.  The parallel-saturation bound is taken at both sides of its edge."""
import ctypes as C
import math
import os
import subprocess

from conftest import ROOT


def test_symbols_structures_and_header(lib):
    from btl_bloomfilter_amd import _lib

    for name in ("btlbf_mibf_build_fastx", "btlbf_mibf_optimal_size", "btlbf_count_windows_seqs",
                 "btlbf_count_windows_fastx"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "btlbf.h")).read()
    assert "BTLBF_MIBF_ID_PER_FILE = 0, BTLBF_MIBF_ID_PER_RECORD = 1" in text
    assert "BTLBF_MIBF_SAT_NONE = 0, BTLBF_MIBF_SAT_SERIAL = 1, BTLBF_MIBF_SAT_PARALLEL = 2" in text
    assert (_lib.MIBF_ID_PER_FILE, _lib.MIBF_ID_PER_RECORD) == (0, 1)
    assert (_lib.MIBF_SAT_NONE, _lib.MIBF_SAT_SERIAL, _lib.MIBF_SAT_PARALLEL) == (0, 1, 2)
    # the structures as the C compiler lays them out (tests/cpp/test_mibf_build_refusals.cpp asserts the same numbers)
    assert C.sizeof(_lib.MibfBuildParams) == 88 and _lib.MibfBuildParams.device.offset == 80
    assert C.sizeof(_lib.MibfBuildReport) == 9 * 8 + 4 * 8 * 4 + 8 and _lib.MibfBuildReport.seconds_total.offset == 200


def test_optimal_size_is_the_references_arithmetic(lib):
    """MIBloomFilter.hpp:84-88 in Python's doubles (the same libm logarithm); a multiple of 64 above the real value"""
    from btl_bloomfilter_amd import MIBloomFilter

    for entries in (0, 1, 63, 6800, 16000, 1200000000, 1 << 40):
        for h in (1, 3, 4, 8):
            for occ in (0.1, 0.3, 0.5, 0.9):
                v = int(-float(entries) * float(h) / math.log(1.0 - occ))
                assert MIBloomFilter.calcOptimalSize(entries, h, occ) == v + (64 - v % 64)
    assert MIBloomFilter.calcOptimalSize(0, 4, 0.5) == 64


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_every_entry_check_answers_before_any_hip_call(tmp_path):
    exe = str(tmp_path / "test_mibf_build_refusals")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wno-unused-function",
                        os.path.join(ROOT, "tests", "cpp", "test_mibf_build_refusals.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all miBF build refusals in place" in r.stdout, r.stdout + r.stderr


def test_example_compiles_and_refuses_without_a_gpu(tmp_path):
    """examples/mibf_build.cpp over the drop-in header: built with g++ against the library; an unreadable reference is
    refused at entry (exit 1, the message names it) whether or not there is a GPU, and no file is written"""
    exe = str(tmp_path / "mibf_build")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "mibf_build.cpp"), "-L" + libdir, "-lbtlbf", "-Wl,-rpath," + libdir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, prefix, "31", "0.3", str(tmp_path / "missing.fa"), "--hashes", "3", "--serial"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "missing.fa" in r.stderr + r.stdout
    assert not any(os.path.exists(prefix + ext) for ext in (".bf", ".mibf", ".ids.tsv"))
    assert subprocess.run([exe, prefix, "31", "0.3", "x.fa"], capture_output=True).returncode == 2  # neither seeds nor hashes
