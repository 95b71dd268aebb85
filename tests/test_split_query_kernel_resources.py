"""The split query's kernels (csrc/split_query_kernels.hip) must compile for gfx950 as a unit of their own, and without
scratch: hipcc's kernel-resource remarks, as in test_mibf_stream_kernel_resources.py, for every kernel of the unit.  The
kernels were part of aux_kernels.hip before; that unit's table showed zero scratch bytes per lane for each of them."""
from kres_util import kernel_resources

# the sampler (straight from global memory / staged in LDS), the prefix sums of the flag words, both ways of moving
# reads and both merges
KERNELS = ["read_sample_kernel<false>", "read_sample_kernel<true>", "flag_chunk_sum_kernel", "flag_chunk_scan_kernel",
           "flag_prefix_kernel", "compact_reads_kernel", "gather_cold_reads_kernel", "merge_split_bitmaps_kernel",
           "merge_cold_bitmaps_kernel"]


def test_split_query_kernels_compile_for_gfx950_without_scratch(tmp_path):
    res = kernel_resources("split_query_kernels.hip", tmp_path / "split_query.o")
    scratch = {k: v["scratch"] for k, v in res.items()}
    print(res)
    assert sorted(scratch) == sorted(KERNELS), scratch
    assert all(v == 0 for v in scratch.values()), scratch
