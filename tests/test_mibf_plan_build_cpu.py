"""The miBF builder's bounds (mibf_parallel_fits / _budget, mibf_batch_windows, mibf_record_room / _budget in
btl_bloomfilter_amd/csrc/mibf_plan.hpp) on the CPU: tests/cpp/test_mibf_plan_build.cpp, a stand-alone program over that
header alone, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

from conftest import ROOT


def test_mibf_build_bounds_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_mibf_plan_build")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           os.path.join(ROOT, "tests", "cpp", "test_mibf_plan_build.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "mibf build plan test passed" in r.stdout
