"""The kernels of csrc/screen_kernels.hip through the compiler's own resource remarks (tests/kres_util.py; hipcc
cross-compiles without a GPU): the expected set of kernels and nothing else, no scratch memory in any of them, and the
LDS each one declares.

Scratch.  screen_kernel keeps per-filter state in arrays indexed by the unrolled filter loop and by the window index; an
index the compiler cannot resolve puts such an array into scratch memory (the second wave of probes did that for five and
more filters while its window loop was a `#pragma unroll` the compiler declined; it is a compile-time index now), and
the spaced-seed instantiations must not take seq_core.hpp's WinHash<true>::hv[32] (they walk the strands with
seq_strand_walk, as the wide-counter kernels do).

LDS, static (the tile and the spaced-seed tables are dynamic LDS and depend on k):
    screen_kernel        sizeof(SeqShared) = 64 x 16 (pair_tab) + 8 x 16 (init_tab) + 256 (lut) + 3 x 8 = 1432, rounded
                         up to its 16-byte alignment: 1440 -- what seq_kernel declares
    screen_tally_kernel  two bins of 32 bits per filter, BTLBF_SCREEN_MAX_FILTERS = 16 of them: 2 x 16 x 4 = 128
    the reduction and the verdict use none

Registers.  Reported, and bounded only where occupancy would fall off a step: 256 threads per workgroup may use up to
512 registers per lane; the widest instantiation (8 filters, plain ntHash: 64 probe words, 16 words of bit indices and 16
of canonical hashes beside the hash stage) must stay within 170, which is three waves per SIMD, and uses no AGPRs."""
import pytest
from kres_util import kernel_resources

NF = range(1, 9)


@pytest.fixture(scope="module")
def screen(tmp_path_factory):
    return kernel_resources("screen_kernels.hip", tmp_path_factory.mktemp("kres") / "screen.o")


def name(nf, spaced):
    return "screen_kernel<%d, %s>" % (nf, "true" if spaced else "false")


def test_the_unit_has_these_kernels_and_no_others(screen):
    names = [name(nf, s) for nf in NF for s in (0, 1)] + ["screen_reduce_kernel", "screen_verdict_kernel", "screen_tally_kernel"]
    assert sorted(names) == sorted(screen), sorted(set(names) ^ set(screen))


def test_no_kernel_uses_scratch(screen):
    bad = {n: r["scratch"] for n, r in screen.items() if r["scratch"] != 0}
    print(bad)
    assert not bad, bad


def test_lds(screen):
    for n, r in screen.items():
        want = 1440 if n.startswith("screen_kernel<") else 2 * 16 * 4 if n == "screen_tally_kernel" else 0
        assert r["lds"] == want, (n, r)


def test_lds_equals_the_single_filter_kernel(screen, tmp_path):
    narrow = kernel_resources("seq_kernels.hip", tmp_path / "seq.o")
    assert narrow["seq_kernel<1, true, false>"]["lds"] == screen[name(1, 0)]["lds"] == 1440


def test_registers(screen):
    for nf in NF:
        for s in (0, 1):
            r = screen[name(nf, s)]
            print(name(nf, s), "vgpr", r["vgpr"], "sgpr", r["sgpr"])
            assert r["vgpr"] <= 170 and r.get("agpr", 0) == 0, (name(nf, s), r)
