"""Build-time guard (no GPU needed: hipcc cross-compiles): the SGPR spill moves inside the candidate-tile loop of
k_scan_skip<false,8>.  On gfx950 a spilled scalar is a lane of a VGPR and every save or restore a VALU instruction; in the
candidate loop they are paid per tile, or per tile and merge, in a phase that is VALU-bound ("Spilled
scalars").  tools/spill_report.py counts them by region on the device assembly; the regression line is what the tree held
before the tile path read its pointers from the argument segment: 22 restores + 12 saves in the loop's own blocks ("cand: per
tile"), 113 + 16 in the own blocks of the loop over a tile's merges ("cand: per tile and merge"; static counts, the rare
straight-to-HBM path of the deltas included).

Figures of the tree that added this guard: per tile 6 + 8 = 14 (bound 34); per tile and merge 35 + 4 = 39 (bound 129;
profiles/README.md, last section)."""
from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

import pytest

from tests import kernel_resources

REPO = Path(__file__).resolve().parent.parent
PARENT = {"cand: per tile": 22 + 12, "cand: per tile and merge": 113 + 16}  # restores + saves


@pytest.fixture(scope="module")
def regions(tmp_path_factory):
    if not Path(kernel_resources.HIPCC).exists():
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("asm") / "yabpe.s"
    flags = re.search(r"^CXXFLAGS \?= (.*)$", (kernel_resources.CSRC / "Makefile").read_text(), re.M).group(1).split()
    out = subprocess.run([kernel_resources.HIPCC, "--offload-arch=gfx950", *flags, "-S", "--offload-device-only", "-o", str(asm), "yabpe.hip"],
                         cwd=kernel_resources.CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = subprocess.run([sys.executable, str(REPO / "tools" / "spill_report.py"), str(asm), "k_scan_skipILb0ELi8E"],
                         capture_output=True, text=True, timeout=300)
    assert rep.returncode == 0, rep.stderr[-2000:]
    found = {}
    for line in rep.stdout.splitlines():  # label, blocks, VALU, scalar, LDS, VMEM, saves, restores, data reads
        m = re.match(r"^(cand: per tile(?: and merge)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            found[m.group(1)] = {"saves": int(m.group(7)), "restores": int(m.group(8))}
    return found


@pytest.mark.parametrize("region", list(PARENT))
def test_candidate_loop_spill_moves_do_not_rise(regions, region):
    assert region in regions, regions
    r = regions[region]
    print(region, r, "bound", PARENT[region])
    assert r["saves"] + r["restores"] <= PARENT[region], (region, r)
