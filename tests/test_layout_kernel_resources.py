"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the fixed-shape batch layouts (yabpe_layout_pad /
yabpe_layout_pack, csrc/yabpe_layout_kernels.h) is there exactly once, uses no scratch memory and (the kernels that share helpers with the
windows and pairs layouts) no more registers than before they shared them."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_lay_lengthsILb0EE", r"_ZN2yb\d+k_lay_lengthsILb1EE", r"_ZN2yb\d+k_lay_pad_writeE", r"_ZN2yb\d+k_lay_pack_writeE"]
VGPRS = {KERNELS[0]: 29, KERNELS[1]: 15, KERNELS[2]: 24}  # lengths<false>, lengths<true>, pad write


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)


def test_no_kernel_needs_more_registers_than_before(resources):
    """Upper bounds: the VGPRs of each kernel before the count kernels shared their tail and the pad write lay_row_col."""
    for k, most in VGPRS.items():
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["VGPRs"] <= most, (k, r)
