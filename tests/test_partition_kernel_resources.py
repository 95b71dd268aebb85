"""The packed instantiations of passes B and C (partition_kernels.hip: 48 entries per 128-byte chunk) must fit a CU as
their unpacked counterparts do: a 1024-thread workgroup needs at most 128 vector registers per lane, and a spill to
scratch would cost the bytes the format saves.  hipcc cross-compiles without a GPU, so the compiler's own
kernel-resource remarks are checked, as tests/test_kernel_resources.py does for pass A."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "btl_bloomfilter_amd", "csrc", "partition_kernels.hip")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "hipcc is part of the image: the build check needs it too"
    obj = tmp_path_factory.mktemp("kres") / "partition_kernels.o"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(obj), SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", cur).replace("void ", "").replace("btlbf::", "")
            out[cur] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur:
                out[cur][key] = int(m.group(1))
    return out


# part_split_kernel<QUERY, EXACT, PK>, part_apply_kernel<MODE, NT, PK> (MODE 0 = bit OR, 1 = bit test)
@pytest.mark.parametrize("kernel", ["part_split_kernel<false, false, true>",
                                    "part_split_kernel<true, false, true>",
                                    "part_apply_kernel<0, 512, true>",
                                    "part_apply_kernel<1, 512, true>",
                                    "part_apply_kernel<0, 1024, true>",
                                    "part_apply_kernel<1, 1024, true>"])
def test_packed_kernels_fit_a_cu(remarks, kernel):
    assert kernel in remarks, sorted(remarks)
    res = remarks[kernel]
    print(kernel, res)
    assert res["vgpr"] <= 128
    assert res["scratch"] == 0, "%s spills %d bytes per lane" % (kernel, res["scratch"])


def test_unpacked_kernels_are_still_built(remarks):
    for kernel in ("part_split_kernel<false, false, false>", "part_split_kernel<false, true, false>",
                   "part_apply_kernel<0, 1024, false>", "part_apply_kernel<2, 512, false>"):
        assert kernel in remarks, sorted(remarks)
