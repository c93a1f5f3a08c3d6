"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels of the fill-in-the-middle feature -- k_fim_plan,
k_fim_write and k_fim_cuts (csrc/yabpe_fim_kernels.h) -- are there exactly once and use no scratch memory, and k_mask, whose
document search and counter shards they share, is as it was.  Their registers and occupancy are recorded in DESIGN.md, not
pinned here."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = [r"_ZN2yb\d+k_fim_planE", r"_ZN2yb\d+k_fim_writeE", r"_ZN2yb\d+k_fim_cutsE"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_every_kernel_once_and_without_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            print(name, r)


def test_the_mask_kernel_is_still_there(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k_maskE", name)]
    assert r["ScratchSize"] == 0
