"""Build-time guard (no GPU needed: hipcc cross-compiles): each kernel of the windows layout (yabpe_layout_windows,
csrc/yabpe_layout_kernels.h) is there exactly once per instantiation and uses no scratch memory."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# (itanium names: template kernels carry their arguments)
KERNELS = [r"_ZN2yb\d+k_lay_win_countE", r"_ZN2yb\d+k_lay_win_rowsE", r"_ZN2yb\d+k_lay_win_writeILb0EE", r"_ZN2yb\d+k_lay_win_writeILb1EE"]


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


def test_no_windows_kernel_uses_scratch_memory(resources):
    for k in KERNELS:
        found = {name: r for name, r in resources.items() if re.match(k, name)}
        assert len(found) == 1, (k, sorted(found))
        for name, r in found.items():
            assert r["ScratchSize"] == 0, (name, r)
            print(name, r)


def test_the_write_kernel_keeps_no_workgroup_state(resources):
    """No LDS and nothing to wait for: a write workgroup reads its rows' records and stores."""
    for k in KERNELS[2:]:
        (r,) = [r for name, r in resources.items() if re.match(k, name)]
        assert r["LDS"] == 0, (k, r)
