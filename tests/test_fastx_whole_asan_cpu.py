"""The parser's BTLBF_FASTX_WHOLE mode under AddressSanitizer and UndefinedBehaviorSanitizer on the host:
tests/cpp/test_fastx_whole.cpp, a stand-alone program linked with csrc/fastx.cpp alone (both built with
-fsanitize=address,undefined -fno-gpu-sanitize: host code only; nothing is loaded into Python, no GPU is used)."""
import os
import subprocess

from conftest import ROOT


def test_fastx_whole_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "test_fastx_whole")
    # host code only: no sanitizer in device code objects
    san = ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function"] + san + \
        [os.path.join(ROOT, "btl_bloomfilter_amd", "csrc", "fastx.cpp"), os.path.join(ROOT, "tests", "cpp", "test_fastx_whole.cpp"),
         "-lz", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path / "reads.fq")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert "fastx whole test passed" in r.stdout
