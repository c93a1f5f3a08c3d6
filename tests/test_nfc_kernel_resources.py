"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the normaliser (yabpe_normalize,
csrc/yabpe_norm_kernels.h) is there exactly once, and the per-byte ones -- the class pass, the three scan kernels, the copy --
use no scratch memory.  The two segment kernels are found and their scratch size printed, not asserted (DESIGN.md (q) records
it: a lane of k_nfc_short or k_nfc_long runs the whole segment routine)."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

PER_BYTE = ["k_nfc_class", "k_nfc_windows", "k_nfc_carry", "k_nfc_apply", "k_nfc_copy", "k_nfc_offsets"]
SEGMENT = ["k_nfc_short", "k_nfc_long"]
# scan kernel -> (VGPRs at most, waves per SIMD at least): what the build reported before the kernels shared yabpe_scan_kernels.h
SCAN_BUDGET = {"k_nfc_windows": (48, 8), "k_nfc_carry": (39, 8), "k_nfc_apply": (56, 8)}


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def found(resources, kernel):
    return {name: r for name, r in resources.items() if re.match(rf"_ZN2yb\d+{kernel}E", name)}


def test_every_kernel_exists_once(resources):
    for k in PER_BYTE + SEGMENT:
        assert len(found(resources, k)) == 1, (k, sorted(found(resources, k)))


def test_per_byte_kernels_use_no_scratch_memory(resources):
    for k in PER_BYTE:
        for name, r in found(resources, k).items():
            assert r["ScratchSize"] == 0, (name, r)
    for k in SEGMENT:
        for name, r in found(resources, k).items():
            print(name, r)


def test_scan_kernels_register_budget(resources):
    for k, (vgprs, waves) in SCAN_BUDGET.items():
        assert len(found(resources, k)) == 1, (k, sorted(found(resources, k)))
        for name, r in found(resources, k).items():
            assert r["VGPRs"] <= vgprs and r["Occupancy"] >= waves, (name, r)
