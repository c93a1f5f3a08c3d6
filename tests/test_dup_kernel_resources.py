"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels of exact-substring deduplication (csrc/yabpe_dup_kernels.h)
are there exactly once and use no scratch memory.  Their registers and occupancy are recorded in DESIGN.md, not pinned here."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources


@pytest.mark.parametrize("kernel", ["k_dup_plan", "k_dup_insert", "k_dup_mark", "k_dup_compact"])
def test_kernel_once_and_without_scratch_memory(kernel):
    found = {name: r for name, r in kernel_resources.resources().items() if re.match(rf"_ZN2yb\d+{kernel}E", name)}
    assert len(found) == 1, (kernel, sorted(found))
    for name, r in found.items():
        assert r["ScratchSize"] == 0, (name, r)
        print(name, r)
