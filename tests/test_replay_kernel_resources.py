"""Build-time guard (no GPU needed: hipcc cross-compiles): the kernels of the resumed load use no scratch memory, and the wave
kernel keeps the registers that let eight waves per SIMD stay resident (it hides the latency of its dependent table reads
with waves)."""
from __future__ import annotations

import re

import pytest

from tests import kernel_resources

KERNELS = ["k_replay_llen", "k_replay_words", "k_load_words_tok", "k_long_lengths_tok", "k_load_long_tok", "k_long_checksum"]


@pytest.fixture(scope="module")
def resources():
    return kernel_resources.resources()


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(rf"_ZN2yb\d+{k}E", name)}
        assert found, k
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)


def test_wave_kernel_keeps_eight_waves_per_simd(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k_replay_wordsE", name)]
    assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8 and r["LDS"] == 0, r
