"""Build-time guard (no GPU needed: hipcc cross-compiles): the tile-centric loader k_load_tiles (csrc/yabpe_kernels.h) and the
gathering retile k_retile_gather (csrc/yabpe_aux_kernels.h) are there exactly once, use no scratch memory and keep the LDS
their occupancy was planned with."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# kernel -> LDS bytes per workgroup it may use (k_load_tiles: image + byte window of four waves, 12,352 B: 8 workgroups per CU;
# k_retile_gather: 8 images + 4 stages, 24,740 B: 6 per CU)
KERNELS = {r"_ZN2yb\d+k_load_tilesE": 16 << 10, r"_ZN2yb\d+k_retile_gatherE": 26 << 10}


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k, lds in KERNELS.items():
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            assert r["LDS"] <= lds, (name, r)
