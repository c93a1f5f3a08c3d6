"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels and instantiations that yabpe_encode_spans adds use no
scratch memory, and the encoder still has its SPANS = false form of k_enc_words."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_enc_wordsILb1EE", r"_ZN2yb\d+k_enc_emit_spansILb0EE", r"_ZN2yb\d+k_enc_emit_spansILb1EE", r"_ZN2yb\d+k_enc_lead_countE"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)


def test_plain_words_kernel_is_still_there_without_scratch(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k_enc_wordsILb0EE", name)]
    assert r["ScratchSize"] == 0, r
