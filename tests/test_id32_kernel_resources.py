"""Build-time guard (no GPU needed: hipcc cross-compiles): no kernel of the u32-id merge loop (yabpe_id32_kernels.h) uses scratch
memory, and the streaming apply keeps the registers, LDS and occupancy DESIGN.md (r) states."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ["k32_count", "k32_count_long", "k32_apply", "k32_apply_long", "k32_select", "k32_rehash", "k32_table_compare", "k32_sum_len",
           "k32_repack", "k32_words", "k32_word_slots", "k32_build_tiles", "k32_place_words"]


@pytest.fixture(scope="module")
def resources():
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    flags = re.search(r"^CXXFLAGS \?= (.*)$", (CSRC / "Makefile").read_text(), re.M).group(1).split()
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "yabpe.hip"],
                         cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def test_no_id32_kernel_uses_scratch_memory(resources):
    names = [n for n in resources if re.match(r"_ZN2yb\d+k32_", n)]
    for k in KERNELS:
        found = {name: resources[name] for name in names if re.match(rf"_ZN2yb\d+{k}(E|I)", name)}
        assert found, k
    for name in names:  # every kernel of the header, listed above or not
        assert resources[name]["ScratchSize"] == 0, (name, resources[name])


def test_streaming_apply_resources(resources):
    (r,) = [r for name, r in resources.items() if re.match(r"_ZN2yb\d+k32_applyE", name)]
    assert (r["VGPRs"], r["Occupancy"], r["LDS"]) == (56, 6, 26176), r
