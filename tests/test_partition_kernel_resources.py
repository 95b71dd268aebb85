"""The packed instantiations of passes B and C (partition_kernels.hip: 48 entries per 128-byte chunk) must fit a CU as
their unpacked counterparts do: a 1024-thread workgroup needs at most 128 vector registers per lane, and a spill to
scratch would cost the bytes the format saves.  hipcc cross-compiles without a GPU, so the compiler's own
kernel-resource remarks are checked, as tests/test_kernel_resources.py does for pass A."""
import pytest
from kres_util import kernel_resources


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    return kernel_resources("partition_kernels.hip", tmp_path_factory.mktemp("kres") / "partition_kernels.o")


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
