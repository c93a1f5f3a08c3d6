"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the o200k_base split pattern (option "split_pattern" = 3,
csrc/yabpe_pretok_kernels.h) is there exactly once, uses no scratch memory and stays within the registers and the occupancy the
build reports today.  The two function-scan kernels are bound by their instructions, so their occupancy of 5 and 4
waves is what they get, not what they need; the others stream bytes once and keep 7 or 8 waves resident."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# kernel -> (VGPRs at most, waves per SIMD at least): what the build reports
BUDGET = {
    r"_ZN2yb\d+k_s5_classE": (26, 8), r"_ZN2yb\d+k_s5_auxE": (20, 8), r"_ZN2yb\d+k_s5_specialE": (13, 8),
    r"_ZN2yb\d+k_la_windowsE": (44, 8), r"_ZN2yb\d+k_la_carryE": (32, 8), r"_ZN2yb\d+k_la_applyE": (72, 7),
    r"_ZN2yb\d+k_fn_windowsE": (87, 5), r"_ZN2yb\d+k_fn_carryE": (52, 8), r"_ZN2yb\d+k_fn_applyE": (102, 4),
}


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def one(resources, pattern):
    found = {name: r for name, r in resources.items() if re.match(pattern, name)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in BUDGET:
        name, r = one(resources, k)
        assert r["ScratchSize"] == 0, (name, r)


def test_register_budget(resources):
    for k, (vgprs, waves) in BUDGET.items():
        name, r = one(resources, k)
        assert r["VGPRs"] <= vgprs and r["Occupancy"] >= waves, (name, r)


def test_the_scan_kernels_hold_no_window_in_lds(resources):
    """Pieces live in registers -- a piece indexed by a loop variable is moved to LDS by the compiler, 8 KiB per workgroup --
    and LDS holds one value per wave for the workgroup's scan (WPB words of 4 or 8 bytes)."""
    for k in BUDGET:
        name, r = one(resources, k)
        assert r["LDS"] <= 64, (name, r)
