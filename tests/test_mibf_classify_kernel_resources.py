"""The classification kernels (csrc/mibf_classify_kernels.hip) must not spill: hipcc's kernel-resource remarks, as in
test_mibf_kernel_resources.py, for every instantiation of the translation unit."""
from kres_util import kernel_resources


def test_mibf_classify_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = {k: v["scratch"] for k, v in kernel_resources("mibf_classify_kernels.hip", tmp_path / "cls.o").items()}
    mine = {k: v for k, v in out.items() if "mibf" in k}
    # the walk with its table in LDS and in global memory x 2 ID types + the largest-id reduction x 2 ID types
    assert len([k for k in mine if "mibf_classify_kernel" in k]) == 4, sorted(mine)
    assert len(mine) == 6, sorted(mine)
    spills = {k: v for k, v in mine.items() if v != 0}
    assert not spills, spills
