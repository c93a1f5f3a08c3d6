"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the normaliser (yabpe_normalize,
csrc/yabpe_norm_kernels.h) is there exactly once, and the per-byte ones -- the class pass, the three scan kernels, the copy --
use no scratch memory.  The two segment kernels are found and their scratch size printed, not asserted (DESIGN.md (q) records
it: a lane of k_nfc_short or k_nfc_long runs the whole segment routine)."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PER_BYTE = ["k_nfc_class", "k_nfc_windows", "k_nfc_carry", "k_nfc_apply", "k_nfc_copy", "k_nfc_offsets"]
SEGMENT = ["k_nfc_short", "k_nfc_long"]


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


def found(resources, kernel):
    return {name: r for name, r in resources.items() if re.match(rf"_ZN2yb\d+{kernel}E", name)}


def test_every_kernel_exists_once(resources):
    for k in PER_BYTE + SEGMENT:
        assert len(found(resources, k)) == 1, (k, sorted(found(resources, k)))


def test_per_byte_kernels_use_no_scratch_memory(resources):
    for k in PER_BYTE:
        for name, r in found(resources, k).items():
            assert r["ScratchSize"] == 0, (name, r)
    for k in SEGMENT:
        for name, r in found(resources, k).items():
            print(name, r)
