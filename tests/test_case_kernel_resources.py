"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of yabpe_lowercase (csrc/yabpe_case_kernels.h) is there
exactly once and uses no scratch memory."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = ["k_case_check", "k_case_same", "k_case_fwd_windows", "k_case_fwd_carry", "k_case_fwd_apply", "k_case_bwd_windows", "k_case_bwd_carry",
           "k_case_bwd_apply", "k_case_write"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def found(resources, kernel):
    return {name: r for name, r in resources.items() if re.match(rf"_ZN2yb\d+{kernel}E", name)}


def test_every_kernel_exists_once(resources):
    for k in KERNELS:
        assert len(found(resources, k)) == 1, (k, sorted(found(resources, k)))


def test_no_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        kernels = found(resources, k)
        assert kernels, k
        for name, r in kernels.items():
            print(name, r)
            assert r["ScratchSize"] == 0, (name, r)
