"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the whole-document packing (yabpe_layout_fit,
csrc/yabpe_fit_kernels.h) is there exactly once and uses no scratch memory; the write kernel's plan window leaves room in LDS for
as many workgroups a CU as its wave slots hold."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_fit_lengthsILb0EE", r"_ZN2yb\d+k_fit_lengthsILb1EE", r"_ZN2yb\d+k_fit_sort_countE", r"_ZN2yb\d+k_fit_sort_scatterE",
           r"_ZN2yb\d+k_fit_writeE"]
LDS_PER_CU, WAVES_PER_CU, WAVES_PER_WORKGROUP = 160 << 10, 32, 4


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_every_kernel_once_and_without_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
    assert sum(1 for name in resources if "k_fit_" in name) == len(KERNELS)


def test_lds_does_not_limit_the_workgroups_of_a_cu(resources):
    for k in KERNELS:
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["LDS"] * (WAVES_PER_CU // WAVES_PER_WORKGROUP) <= LDS_PER_CU, (k, r)
