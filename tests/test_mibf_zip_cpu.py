"""The mates zipper of the file classifier (btl_bloomfilter_amd/csrc/mibf_zip.hpp) on the CPU: tests/cpp/test_mibf_zip.cpp,
a stand-alone program over that header alone, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

from conftest import ROOT


def test_mibf_zip_against_the_index_wise_zip(tmp_path):
    exe = str(tmp_path / "test_mibf_zip")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           os.path.join(ROOT, "tests", "cpp", "test_mibf_zip.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "mibf zip test passed" in r.stdout
