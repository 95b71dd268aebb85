"""The file classifier's device helpers (csrc/mibf_stream_kernels.hip) must compile for gfx950 without scratch: hipcc's
kernel-resource remarks, as in test_mibf_classify_pair_kernel_resources.py, for every kernel of the translation unit."""
from kres_util import kernel_resources


def test_mibf_stream_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources("mibf_stream_kernels.hip", tmp_path / "stream.o")
    out = {k: v["scratch"] for k, v in res.items()}
    lds = {k: v["lds"] for k, v in res.items()}
    print(out, lds)
    # the copy kernel and the tally kernel, and nothing else
    assert len(out) == 2 and any("interleave_mates_kernel" in k for k in out) and any("mibf_tally_kernel" in k for k in out)
    assert all(v == 0 for v in out.values()), out
    # the tally's workgroup bins: best and any, 8192 ids of 32 bits each; the copy kernel uses no LDS
    assert sorted(lds.values()) == [0, 2 * 8192 * 4], lds
