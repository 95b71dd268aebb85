"""The miBF builder's device helpers (csrc/mibf_build_kernels.hip) must compile for gfx950 without scratch: hipcc's
kernel-resource remarks, as in test_mibf_stream_kernel_resources.py, for every kernel of the translation unit."""
from kres_util import kernel_resources


def test_mibf_build_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources("mibf_build_kernels.hip", tmp_path / "build.o")
    out = {k: v["scratch"] for k, v in res.items()}
    lds = {k: v["lds"] for k, v in res.items()}
    print(out, lds)
    # the window counter and the id helper, and nothing else
    assert len(out) == 2 and any("count_windows_kernel" in k for k in out) and any("mibf_fill_ids_kernel" in k for k in out)
    assert all(v == 0 for v in out.values()), out
    # the counter's block reduction: two sums of four wavefronts, 64 bits each; the id helper uses no LDS
    assert sorted(lds.values()) == [0, 2 * 4 * 8], lds
