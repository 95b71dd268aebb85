"""The C++ drop-in shim CountingBloomFilter<T> for T = uint64_t, uint16_t and uint32_t: the reference's own unit test
(Tests/Unit/CountingBloomFilterTests.cpp: setup, "query elements", "save/load 64 bit Bloom file") replayed through it by
tests/cpp/test_shims_wide.cpp, in the style of tests/test_gpu_cpp_shims.py."""
import os
import subprocess

import pytest
from conftest import ROOT


def build_program(tmp_path):
    from btl_bloomfilter_amd import build

    build.build()
    exe = str(tmp_path / "test_shims_wide")
    libdir = os.path.join(ROOT, "btl_bloomfilter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "test_shims_wide.cpp"), "-L" + libdir, "-lbtlbf",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_wide_shim_test_compiles_on_cpu(tmp_path):
    assert os.path.exists(build_program(tmp_path))


@pytest.mark.gpu
def test_reference_unit_test_through_the_wide_shims(tmp_path):
    r = subprocess.run([build_program(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all wide shim tests passed" in r.stdout
