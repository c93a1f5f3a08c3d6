"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels that yabpe_encode_dropout adds use no scratch (private)
memory and no LDS, and the merge kernel keeps the registers of a full-occupancy wave within reach."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_drop_wordsILb0EE", r"_ZN2yb\d+k_drop_wordsILb1EE", r"_ZN2yb\d+k_drop_long_listE", r"_ZN2yb\d+k_drop_longE",
           r"_ZN2yb\d+k_drop_long_emitE"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_dropout_kernel_uses_scratch_memory_or_lds(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0 and r["LDS"] == 0, (name, r)


def test_merge_kernel_keeps_its_occupancy(resources):
    """k_drop_words hides its table lookups behind other waves: at most 72 VGPRs (7 waves per SIMD of the 512 a lane has)."""
    for k in KERNELS[:2]:
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (k, r)
