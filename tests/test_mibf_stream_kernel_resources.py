"""The file classifier's device helpers (csrc/mibf_stream_kernels.hip) must compile for gfx950 without scratch: hipcc's
kernel-resource remarks, as in test_mibf_classify_pair_kernel_resources.py, for every kernel of the translation unit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "btl_bloomfilter_amd", "csrc", "mibf_stream_kernels.hip")


def test_mibf_stream_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "stream.o"), SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, lds, cur = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = None
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            out[cur] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and cur:
            lds[cur] = int(m.group(1))
    print(out, lds)
    # the copy kernel and the tally kernel, and nothing else
    assert len(out) == 2 and any("interleave_mates_kernel" in k for k in out) and any("mibf_tally_kernel" in k for k in out)
    assert all(v == 0 for v in out.values()), out
    # the tally's workgroup bins: best and any, 8192 ids of 32 bits each; the copy kernel uses no LDS
    assert sorted(lds.values()) == [0, 2 * 8192 * 4], lds
