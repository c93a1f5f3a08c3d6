"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels of the masked-language-model feature -- k_mask
(csrc/yabpe_mask_kernels.h) and the word-index form of the emit pass, k_enc_emit_words (csrc/yabpe_encode_kernels.h) -- are
there exactly once and use no scratch memory, and the encoder keeps its plain emit kernel.  Their registers and occupancy are
recorded in DESIGN.md, not pinned here."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = [r"_ZN2yb\d+k_maskE", r"_ZN2yb\d+k_enc_emit_wordsE"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_every_kernel_once_and_without_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            print(name, r)


def test_the_plain_emit_pass_is_still_there(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k_enc_emitE", name)]
    assert r["ScratchSize"] == 0
