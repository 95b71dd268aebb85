"""The kernels of csrc/card_kernels.hip through the compiler's own resource remarks (tests/kres_util.py, what
tools/kres.py prints; hipcc cross-compiles without a GPU): none uses scratch memory, the fused kernel keeps the sequence
kernels' four waves per SIMD and their static LDS, and the unit holds the kernels the design names and no others."""
import pytest
from kres_util import kernel_resources

KERNELS = ["card_kernel", "card_fix_kernel", "card_hist_kernel", "card_merge_kernel"]


@pytest.fixture(scope="module")
def card(tmp_path_factory):
    return kernel_resources("card_kernels.hip", tmp_path_factory.mktemp("kres") / "card.o")


def test_the_unit_has_its_kernels(card):
    assert sorted(card) == sorted(KERNELS), sorted(card)


@pytest.mark.parametrize("name", KERNELS)
def test_no_kernel_uses_scratch(card, name):
    print(name, card[name])
    assert card[name]["scratch"] == 0, card[name]


def test_the_fused_kernel_keeps_four_waves_per_simd(card):
    r = card["card_kernel"]
    assert r["vgpr"] <= 128 and r.get("agpr", 0) == 0, r
    # SeqShared and the workgroup's two counters: inside what internal.hpp reserves as the sequence kernels' static LDS
    assert r["lds"] <= 1536, r
