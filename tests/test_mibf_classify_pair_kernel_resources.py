"""The paired classification kernels (csrc/mibf_classify_pair_kernels.hip) must not spill: hipcc's kernel-resource
remarks, as in test_mibf_classify_kernel_resources.py, for every instantiation of the translation unit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "btl_bloomfilter_amd", "csrc", "mibf_classify_pair_kernels.hip")


def test_mibf_classify_pair_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "clsp.o"), SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = None
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur] = int(m.group(1))
    mine = {k: v for k, v in out.items() if "mibf" in k}
    # the paired walk with its table in LDS and in global memory x 2 ID types, and nothing else
    assert len([k for k in mine if "mibf_classify_pair_kernel" in k]) == 4, sorted(mine)
    assert len(mine) == 4, sorted(mine)
    spills = {k: v for k, v in mine.items() if v != 0}
    assert not spills, spills
