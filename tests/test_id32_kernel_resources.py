"""Build-time guard (no GPU needed: hipcc cross-compiles): no kernel of the u32-id merge loop (yabpe_id32_kernels.h) uses scratch
memory, and the streaming apply keeps the registers, LDS and occupancy DESIGN.md (r) states."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = ["k32_count", "k32_count_long", "k32_apply", "k32_apply_long", "k32_select", "k32_rehash", "k32_table_compare", "k32_sum_len",
           "k32_repack", "k32_words", "k32_word_slots", "k32_build_tiles", "k32_place_words"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_id32_kernel_uses_scratch_memory(resources):
    names = [n for n in resources if re.match(r"_ZN2yb\d+k32_", n)]
    for k in KERNELS:
        found = {name: resources[name] for name in names if re.match(rf"_ZN2yb\d+{k}(E|I)", name)}
        assert found, k
    for name in names:  # every kernel of the header, listed above or not
        assert resources[name]["ScratchSize"] == 0, (name, resources[name])


def test_streaming_apply_resources(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k32_applyE", name)]
    assert (r["VGPRs"], r["Occupancy"], r["LDS"]) == (56, 6, 26176), r
