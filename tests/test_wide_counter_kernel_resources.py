"""The kernels of csrc/wide_counter_kernels.hip through the compiler's own resource remarks (tests/kres_util.py; hipcc
cross-compiles without a GPU).

Scratch.  No kernel of the unit uses scratch memory.  The spaced-seed instantiations are the ones to watch: the shared
hash stage hands a window's h values over as WinHash<true>::hv[32] (seq_core.hpp), which with a run-time hash count is
indexed at run time and then lives in scratch -- 288 bytes per lane in every spaced-seed instantiation of the 8-bit
seq_kernel.  The wide kernels do not take that array: they produce a window's values one at a time and probe each at
once (wide_spaced_walk in the unit).

Registers.  A wide instantiation may use no more vector registers than the matching 8-bit seq_kernel instantiation
(OP_CBF_QUERY / OP_CBF_INC_ALL / OP_CBF_INC_MIN with the same POW2 and SPACED), compiled here from the same tree, plus a
margin.  Measured (8-bit -> 16 / 32 / 64 bits; pow2, not pow2; plain ntHash):
    query         46, 49 -> 79, 79 / 78, 79 / 109, 111
    incrementAll  46, 46 -> 46, 46 / 46, 46 / 46, 46
    incrementMin 201, 204 -> 46, 47 / 46, 47 / 46, 49   (the 8-bit kernel is the fetched-words variant)
and with spaced seeds: query 55, 51 -> 49, 51 for every width; incrementAll 47, 45 -> 43, 44; incrementMin 47, 45 ->
at most 45, 47.  The margin: 8 registers, one allocation granule of the register file (below it occupancy cannot
change), for every kernel; and for the plain-ntHash query the pipeline buffer that issuing all h loads of a lane's 8
windows before the first is consumed needs and the 8-bit OP_CBF_QUERY (which probes window by window) does not have:
8 windows x 4 loads x 1 register (16 / 32 bits) or x 2 registers (64 bits) = 32 or 64.  Every wide kernel stays at or
below 128 registers: four waves per SIMD, as the 8-bit kernels' launch bounds give."""
import pytest
from kres_util import kernel_resources

OPS = {0: 5, 1: 4, 2: 3}  # W_QUERY, W_INC_ALL, W_INC_MIN -> OP_CBF_QUERY, OP_CBF_INC_ALL, OP_CBF_INC_MIN
GRANULE = 8


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return kernel_resources("wide_counter_kernels.hip", tmp_path_factory.mktemp("kres") / "wide.o")


@pytest.fixture(scope="module")
def narrow(tmp_path_factory):
    return kernel_resources("seq_kernels.hip", tmp_path_factory.mktemp("kres") / "seq.o")


def tf(b):
    return "true" if b else "false"


def test_the_unit_has_every_instantiation(wide):
    names = ["wide_seq_kernel<%d, %d, %s, %s>" % (op, b, tf(p), tf(s)) for op in OPS for b in (2, 4, 8) for p in (1, 0)
             for s in (0, 1)]
    names += ["wide_rows_kernel<%d, %s>" % (b, tf(p)) for b in (2, 4, 8) for p in (1, 0)]
    names += ["wide_rows_serial_kernel<%d, %s>" % (b, tf(p)) for b in (2, 4, 8) for p in (1, 0)]
    names += ["wide_popcount_kernel<%d>" % b for b in (2, 4, 8)] + ["wide_compare_kernel<%d>" % b for b in (2, 4, 8)]
    assert sorted(names) == sorted(wide), sorted(set(names) ^ set(wide))
    assert len([n for n in wide if n.startswith("wide_seq_kernel")]) == 36  # 3 ops x 3 widths x 4


def test_no_kernel_uses_scratch(wide):
    bad = {n: r["scratch"] for n, r in wide.items() if r["scratch"] != 0}
    print(bad)
    assert not bad, bad


def test_plain_nthash_kernels_and_row_kernels_and_reductions_use_no_scratch(wide):
    for n, r in wide.items():
        if not n.endswith(", true>") or not n.startswith("wide_seq_kernel"):
            assert r["scratch"] == 0, (n, r)


@pytest.mark.parametrize("spaced", [0, 1], ids=["nthash", "spaced"])
@pytest.mark.parametrize("pow2", [1, 0], ids=["pow2", "mod"])
@pytest.mark.parametrize("nbytes", [2, 4, 8])
@pytest.mark.parametrize("op", list(OPS))
def test_registers_against_the_8_bit_kernel(wide, narrow, op, nbytes, pow2, spaced):
    w = wide["wide_seq_kernel<%d, %d, %s, %s>" % (op, nbytes, tf(pow2), tf(spaced))]
    n = narrow["seq_kernel<%d, %s, %s>" % (OPS[op], tf(pow2), tf(spaced))]
    margin = GRANULE + (8 * 4 * (2 if nbytes == 8 else 1) if op == 0 and not spaced else 0)
    print(op, nbytes, pow2, spaced, "wide", w["vgpr"], "8-bit", n["vgpr"], "margin", margin)
    assert w["vgpr"] <= n["vgpr"] + margin
    assert w["vgpr"] <= 128 and w.get("agpr", 0) == 0
    assert w["lds"] == n["lds"]
