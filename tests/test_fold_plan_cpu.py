"""The host arithmetic of the filter algebra without a GPU: csrc/fold_plan.hpp (refusals, result size, groups that cover
every slice once, the bound on the scratch) and csrc/algebra_swar.hpp (the packed saturating add / max / min / compare
and the unaligned read that algebra_kernels.hip is made of) against brute force, under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/cpp/test_fold_plan.cpp, a stand-alone program)."""
import os
import subprocess

from conftest import ROOT


def test_fold_plan_and_packed_arithmetic_against_brute_force(tmp_path):
    exe = str(tmp_path / "test_fold_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           os.path.join(ROOT, "tests", "cpp", "test_fold_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert "fold plan test passed" in r.stdout
