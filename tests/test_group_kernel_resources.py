"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the digit-group pass (option "digit_group",
csrc/yabpe_pretok_kernels.h) is there exactly once and uses no scratch memory."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = [r"_ZN2yb\d+k_grp_windowsE", r"_ZN2yb\d+k_grp_carryE", r"_ZN2yb\d+k_grp_applyE"]
# kernel -> (VGPRs at most, waves per SIMD at least): what the build reported before the kernels shared yabpe_scan_kernels.h
BUDGET = {r"_ZN2yb\d+k_grp_windowsE": (26, 8), r"_ZN2yb\d+k_grp_carryE": (24, 8), r"_ZN2yb\d+k_grp_applyE": (34, 8)}


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)


def test_register_budget(resources):
    for k, (vgprs, waves) in BUDGET.items():
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["VGPRs"] <= vgprs and r["Occupancy"] >= waves, (name, r)
