"""What the compiler reports for every kernel of csrc/yabpe.hip, for the build-time resource guards (test_*kernel_resources.py).
No GPU needed: hipcc cross-compiles for gfx950.  One compile per process, whichever guard asks first."""
from __future__ import annotations

import functools
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "yet-another-bpe_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@functools.lru_cache(maxsize=None)
def _compile():
    flags = re.search(r"^CXXFLAGS \?= (.*)$", (CSRC / "Makefile").read_text(), re.M).group(1).split()
    return subprocess.run([HIPCC, "--offload-arch=gfx950", *flags, "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "yabpe.hip"],
                          cwd=CSRC, capture_output=True, text=True, timeout=900)


def resources():
    """mangled kernel name -> {"VGPRs", "ScratchSize", "Occupancy", "LDS"}, with the flags of csrc/Makefile."""
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = _compile()
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
