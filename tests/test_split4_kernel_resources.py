"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the cl100k split pattern (option "split_pattern",
csrc/yabpe_pretok_kernels.h) is there exactly once, uses no scratch memory and stays within the register budget its launch
assumes.  A SIMD has 512 VGPRs per lane: the three scan kernels stream meta and flags once and hide the latency with 8
resident waves (<= 64 VGPRs); the local and the special pass keep the 7 waves of their GPT-2 twins (<= 72 VGPRs)."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

SCAN = [r"_ZN2yb\d+k_nl_windowsE", r"_ZN2yb\d+k_nl_carryE", r"_ZN2yb\d+k_nl_applyE"]
LOCAL = [r"_ZN2yb\d+k_pt4_fusedE", r"_ZN2yb\d+k_pt4_specialE"]
TWINS = [r"_ZN2yb\d+k_pt_fusedE", r"_ZN2yb\d+k_pt_specialE"]
# scan kernel -> (VGPRs at most, waves per SIMD at least): what the build reported before the kernels shared yabpe_scan_kernels.h
SCAN_BUDGET = {r"_ZN2yb\d+k_nl_windowsE": (40, 8), r"_ZN2yb\d+k_nl_carryE": (40, 8), r"_ZN2yb\d+k_nl_applyE": (47, 8)}


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def one(resources, pattern):
    found = {name: r for name, r in resources.items() if re.match(pattern, name)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in SCAN + LOCAL:
        name, r = one(resources, k)
        assert r["ScratchSize"] == 0, (name, r)


def test_register_budget(resources):
    for k in SCAN:
        name, r = one(resources, k)
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (name, r)
    for k, (vgprs, waves) in SCAN_BUDGET.items():
        name, r = one(resources, k)
        assert r["VGPRs"] <= vgprs and r["Occupancy"] >= waves, (name, r)
    for k in LOCAL:
        name, r = one(resources, k)
        assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (name, r)


def test_the_gpt2_kernels_are_still_there_once(resources):
    """The GPT-2 passes keep their names and arguments next to the new ones, the same LDS, and no scratch."""
    for k, twin in zip(TWINS, LOCAL):
        name, r = one(resources, k)
        assert name.endswith("ENS_12PretokParamsE") and r["ScratchSize"] == 0, (name, r)
        assert r["LDS"] == one(resources, twin)[1]["LDS"]
