"""The miBF kernels (csrc/mibf_kernels.hip) must not spill: hipcc's kernel-resource remarks, as in
test_kernel_resources.py, for every instantiation of the translation unit."""
from kres_util import kernel_resources


def test_mibf_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = {k: v["scratch"] for k, v in kernel_resources("mibf_kernels.hip", tmp_path / "mibf.o").items()}
    mine = {k: v for k, v in out.items() if "mibf" in k}
    # 3 window kernels x 9 hash configurations x 2 ID types + 6 kernels x 2 ID types
    assert len([k for k in mine if "mibf_seq_kernel" in k]) == 54, sorted(mine)
    assert len(mine) == 66, sorted(mine)
    spills = {k: v for k, v in mine.items() if v != 0}
    assert not spills, spills
