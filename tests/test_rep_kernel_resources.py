"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels of the repetition signals (csrc/yabpe_rep_kernels.h) are
there exactly once and use no scratch memory, and the LDS form's static LDS stays within 64 KiB.  Their registers and
occupancy are recorded in DESIGN.md, not pinned here."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources


@pytest.mark.parametrize("kernel", ["k_rep_plan", "k_rep_short", "k_rep_insert", "k_rep_mark"])
def test_kernel_once_and_without_scratch_memory(kernel):
    found = {name: r for name, r in kernel_resources.resources().items() if re.match(rf"_ZN2yb\d+{kernel}E", name)}
    assert len(found) == 1, (kernel, sorted(found))
    for name, r in found.items():
        assert r["ScratchSize"] == 0, (name, r)
        assert kernel != "k_rep_short" or 0 < r["LDS"] <= 64 << 10, (name, r)
        print(name, r)
