"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the pairs layout (yabpe_layout_pairs,
csrc/yabpe_layout_kernels.h) is there exactly once per instantiation, uses no scratch memory and no more registers than before the
write kernel became the one it shares with the windows layout."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_lay_pair_countE", r"_ZN2yb\d+k_lay_pair_rowsE", r"_ZN2yb\d+k_lay_rows_writeINS_\d+LayPairRowELb0EE",
           r"_ZN2yb\d+k_lay_rows_writeINS_\d+LayPairRowELb1EE"]
VGPRS = {KERNELS[0]: 29, KERNELS[2]: 28, KERNELS[3]: 42}  # count, write, write with spans


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_pairs_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            print(name, r)


def test_the_write_kernel_keeps_no_workgroup_state(resources):
    """No LDS and nothing to wait for: a write workgroup reads its rows' records and stores."""
    for k in KERNELS[2:]:
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["LDS"] == 0, (k, r)


def test_no_kernel_needs_more_registers_than_before(resources):
    """Upper bounds: the VGPRs of each kernel before windows and pairs shared their write kernel."""
    for k, most in VGPRS.items():
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["VGPRs"] <= most, (k, r)
