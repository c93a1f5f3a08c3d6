"""Build-time guard (no GPU needed: hipcc cross-compiles): the tile-centric loader k_load_tiles (csrc/yabpe_kernels.h) and the
gathering retile k_retile_gather (csrc/yabpe_aux_kernels.h) are there exactly once, use no scratch memory and keep the LDS
their occupancy was planned with."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# kernel -> LDS bytes per workgroup it may use (k_load_tiles: image + byte window of four waves, 12,352 B: 8 workgroups per CU;
# k_retile_gather: 8 images + 4 stages, 24,740 B: 6 per CU)
KERNELS = {r"_ZN2yb\d+k_load_tilesE": 16 << 10, r"_ZN2yb\d+k_retile_gatherE": 26 << 10}


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


def test_no_new_kernel_uses_scratch_memory(resources):
    for k, lds in KERNELS.items():
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            assert r["LDS"] <= lds, (name, r)
