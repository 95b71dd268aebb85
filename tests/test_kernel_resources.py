"""The benchmark's pass-A kernels must not spill: a change that pushes them over their 128 vector registers shows up
as 3 ms per launch on the GPU (the overflow path's bin-width constants, the ragged / mask code compiled into
every variant) and as nothing at all in the parity tests.  hipcc cross-compiles without a GPU, so the compiler's own
kernel-resource remarks are checked here for the h = 4 translation unit (tools/kres.py prints the whole table)."""
import pytest
from kres_util import kernel_resources


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    return kernel_resources("part_hash_inst.hip", tmp_path_factory.mktemp("kres") / "part_hash_h4.o", ["-DBTLBF_PART_H=4"])


# <H, POW2, SPACED, QUERY, WINDOW, AUX>
@pytest.mark.parametrize("kernel", ["part_hash_ov_kernel<4, true, false, false, false, false>",   # C2 insert
                                    "part_hash_ov_kernel<4, true, false, true, false, false>",    # C2 query
                                    "part_hash_ov_kernel<4, true, false, false, false, true>"])   # ragged insert
def test_headline_pass_a_kernels_do_not_spill(remarks, kernel):
    assert kernel in remarks, sorted(remarks)[:5]
    res = remarks[kernel]
    assert res["vgpr"] <= 128
    assert res["scratch"] == 0, "%s spills %d bytes per lane: python tools/kres.py part_hash_inst.hip -DBTLBF_PART_H=4" % (kernel, res["scratch"])
