"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the persistent word pool (yabpe_pool_add,
csrc/yabpe_pool_kernels.h) is there exactly once and uses no scratch memory."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = [r"_ZN2yb\d+k_pool_compactE", r"_ZN2yb\d+k_pool_probeE", r"_ZN2yb\d+k_pool_appendE", r"_ZN2yb\d+k_pool_rehashE"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
