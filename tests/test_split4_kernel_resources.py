"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the cl100k split pattern (option "split_pattern",
csrc/yabpe_pretok_kernels.h) is there exactly once, uses no scratch memory and stays within the register budget its launch
assumes.  A SIMD has 512 VGPRs per lane: the three scan kernels stream meta and flags once and hide the latency with 8
resident waves (<= 64 VGPRs); the local and the special pass keep the 7 waves of their GPT-2 twins (<= 72 VGPRs)."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SCAN = [r"_ZN2yb\d+k_nl_windowsE", r"_ZN2yb\d+k_nl_carryE", r"_ZN2yb\d+k_nl_applyE"]
LOCAL = [r"_ZN2yb\d+k_pt4_fusedE", r"_ZN2yb\d+k_pt4_specialE"]
TWINS = [r"_ZN2yb\d+k_pt_fusedE", r"_ZN2yb\d+k_pt_specialE"]


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


def one(resources, pattern):
    found = {name: r for name, r in resources.items() if re.match(pattern, name)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def test_no_new_kernel_uses_scratch_memory(resources):
    for k in SCAN + LOCAL:
        name, r = one(resources, k)
        assert r["ScratchSize"] == 0, (name, r)


def test_register_budget(resources):
    for k in SCAN:
        name, r = one(resources, k)
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (name, r)
    for k in LOCAL:
        name, r = one(resources, k)
        assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (name, r)


def test_the_gpt2_kernels_are_still_there_once(resources):
    """The GPT-2 passes keep their names and arguments next to the new ones, the same LDS, and no scratch."""
    for k, twin in zip(TWINS, LOCAL):
        name, r = one(resources, k)
        assert name.endswith("ENS_12PretokParamsE") and r["ScratchSize"] == 0, (name, r)
        assert r["LDS"] == one(resources, twin)[1]["LDS"]
