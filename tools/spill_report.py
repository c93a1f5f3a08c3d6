#!/usr/bin/env python3
"""Where the SGPR spill moves of a kernel sit: per basic block, per loop, and on the candidate-tile path of k_scan_skip.

On gfx950 a spilled SGPR is a lane of a VGPR: the save is a v_writelane_b32, the restore a v_readlane_b32 -- VALU
instructions with a scalar dependency behind them.  The static total says little (single_site_tile reads lanes of the
TILE on purpose, and a save at kernel entry is paid once per launch); what matters is how many of them execute per
candidate tile.  This tool reads the assembly text of one kernel and lists the moves where they are.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> -S --offload-device-only -o yabpe.s yabpe.hip
    python tools/spill_report.py yabpe.s 'k_scan_skipILb0ELi8E' > profiles/spill_report_parent.txt

Text only.  It knows the lane moves (v_writelane_b32 / v_readlane_b32), the instruction-class prefixes (v_ VALU, s_
scalar, ds_ LDS, global_/buffer_/flat_/scratch_ vector memory), and branches as far as the control-flow graph needs them
(s_branch, s_cbranch_*, s_endpgm).  A SPILL VGPR is the destination of a v_writelane_b32 that no other instruction names as
an operand; every other lane read is a DATA read (neighbour fetch, prefix totals).

Regions.  Loops are the natural loops of the control-flow graph (dominators, back edges).  The CANDIDATE loop is found by
what only it does: among the loops nested directly inside a top-level loop, the one with the most data lane reads (the
neighbour fetches of single_site_tile).  Its parent is the CHUNK loop; the blocks of the chunk loop in front of the
candidate loop are the signature sweep, those behind it the chunk's end (claiming the next piece), and everything behind
the chunk loop is the flush, the ticket and the selection tail.  --candidate-loop LABEL overrides the choice.  Inside the
candidate loop the blocks are split by nesting: the loop's own blocks (claim, prefetch, write-back: per TILE), the own
blocks of the loop over the merges a tile was noted for (match, single_site_tile, the straight parts of slow_tile: per
tile and MERGE), and the loops nested deeper (aggregator probes, slow_tile's site walk).

--blocks A,B,C sums a path that was read off the listing (block names as printed), so that a per-path figure in a
document can be reproduced.
"""
from __future__ import annotations

import argparse
import re
import sys
from collections import defaultdict

VMEM_PREFIXES = ("global_", "buffer_", "flat_", "scratch_")
LABEL_RE = re.compile(r"^(\.LBB\d+_\d+):")
FALL_RE = re.compile(r"^;\s*%bb\.(\d+):")
VREG_RE = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


class Block:
    def __init__(self, name: str, line: int):
        self.name, self.line = name, line
        self.ins: list[tuple[str, str]] = []  # (mnemonic, operands)
        self.succ: list[str] = []
        self.falls = True  # control reaches the next block in layout order
        self.valu = self.scalar = self.lds = self.vmem = 0
        self.save = self.restore = self.data_rd = self.data_wr = 0


def kernel_lines(path: str, name: str) -> tuple[str, list[tuple[int, str]]]:
    """The lines of the one function whose symbol contains `name` (line number, text)."""
    out: list[tuple[int, str]] = []
    sym = None
    with open(path, encoding="utf-8", errors="replace") as f:
        for no, raw in enumerate(f, 1):
            if sym is None:
                m = re.match(r"^([A-Za-z_][\w$.]*):", raw)
                if m and name in m.group(1) and not m.group(1).startswith(".L"):
                    sym = m.group(1)
                continue
            if raw.startswith(".Lfunc_end"):
                break
            out.append((no, raw.rstrip("\n")))
    if sym is None:
        sys.exit(f"no function whose symbol contains {name!r} in {path}")
    return sym, out


def vregs(operand: str) -> set[int]:
    regs: set[int] = set()
    for m in VREG_RE.finditer(operand):
        if m.group(1) is not None:
            regs.add(int(m.group(1)))
        else:
            regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return regs


def parse(lines: list[tuple[int, str]]) -> list[Block]:
    blocks = [Block("entry", lines[0][0] if lines else 0)]
    for no, raw in lines:
        m = LABEL_RE.match(raw)
        if m:
            blocks.append(Block(m.group(1), no))
            continue
        m = FALL_RE.match(raw.strip())
        if m:
            blocks.append(Block(f"%bb.{m.group(1)}", no))
            continue
        text = raw.split(";", 1)[0].strip()
        if not text or text.startswith(".") or text.endswith(":"):
            continue
        parts = text.split(None, 1)
        blocks[-1].ins.append((parts[0], parts[1] if len(parts) > 1 else ""))
    return [b for b in blocks if b.ins or b.name != "entry"]


def find_spill_vgprs(blocks: list[Block]) -> set[int]:
    written: set[int] = set()
    used_elsewhere: set[int] = set()
    for b in blocks:
        for mn, ops in b.ins:
            o = [x.strip() for x in ops.split(",")]
            if mn.startswith("v_writelane_b32"):
                written |= vregs(o[0])
                for x in o[1:]:
                    used_elsewhere |= vregs(x)
            elif mn.startswith("v_readlane_b32"):
                used_elsewhere |= vregs(o[0])  # (the destination is scalar; the source may be a spill VGPR)
                for x in o[2:]:
                    used_elsewhere |= vregs(x)
            else:
                used_elsewhere |= vregs(ops)
    return written - used_elsewhere


def classify(blocks: list[Block], spill: set[int]) -> None:
    for i, b in enumerate(blocks):
        for mn, ops in b.ins:
            o = [x.strip() for x in ops.split(",")]
            if mn.startswith("v_"):
                b.valu += 1
                if mn.startswith("v_writelane_b32"):
                    if vregs(o[0]) & spill:
                        b.save += 1
                    else:
                        b.data_wr += 1
                elif mn.startswith("v_readlane_b32"):
                    if vregs(o[1]) & spill:
                        b.restore += 1
                    else:
                        b.data_rd += 1
            elif mn.startswith("s_"):
                b.scalar += 1
                if mn == "s_branch":
                    b.succ.append(o[0])
                    b.falls = False
                elif mn.startswith("s_cbranch_"):
                    b.succ.append(o[-1])
                elif mn.startswith("s_endpgm"):
                    b.falls = False
            elif mn.startswith("ds_"):
                b.lds += 1
            elif mn.startswith(VMEM_PREFIXES):
                b.vmem += 1
        if b.falls and i + 1 < len(blocks):
            b.succ.append(blocks[i + 1].name)


def loops_of(blocks: list[Block]):
    """Natural loops: {header index: set of block indices}, from dominators over the blocks reachable from the entry."""
    idx = {b.name: i for i, b in enumerate(blocks)}
    succ = [[idx[s] for s in b.succ if s in idx] for b in blocks]
    n = len(blocks)
    order: list[int] = []
    seen = [False] * n
    stack = [(0, iter(succ[0]))]
    seen[0] = True
    while stack:  # (iterative depth-first walk: the kernel has thousands of blocks)
        v, it = stack[-1]
        for w in it:
            if not seen[w]:
                seen[w] = True
                stack.append((w, iter(succ[w])))
                break
        else:
            order.append(v)
            stack.pop()
    rpo = order[::-1]
    pos = {v: i for i, v in enumerate(rpo)}
    pred: list[list[int]] = [[] for _ in range(n)]
    for v in rpo:
        for w in succ[v]:
            pred[w].append(v)
    idom = {0: 0}
    changed = True
    while changed:  # (Cooper, Harvey, Kennedy)
        changed = False
        for v in rpo[1:]:
            new = None
            for p in pred[v]:
                if p not in idom:
                    continue
                if new is None:
                    new = p
                    continue
                a, b = p, new
                while a != b:
                    while pos[a] > pos[b]:
                        a = idom[a]
                    while pos[b] > pos[a]:
                        b = idom[b]
                new = a
            if new is not None and idom.get(v) != new:
                idom[v] = new
                changed = True

    def dominates(h: int, v: int) -> bool:
        while True:
            if v == h:
                return True
            if v == 0:
                return False
            v = idom[v]

    loops: dict[int, set[int]] = defaultdict(set)
    for v in rpo:
        for h in succ[v]:
            if h in idom and dominates(h, v):
                body = {h}
                work = [v]
                while work:
                    x = work.pop()
                    if x in body:
                        continue
                    body.add(x)
                    work.extend(p for p in pred[x] if p in idom)
                loops[h] |= body
    return dict(loops), set(rpo)


FIELDS = ("valu", "scalar", "lds", "vmem", "save", "restore", "data_rd")


def total(blocks: list[Block], members) -> dict[str, int]:
    return {f: sum(getattr(blocks[i], f) for i in members) for f in FIELDS}


def row(label: str, n_blocks: int, t: dict[str, int]) -> str:
    return (f"{label:<46} {n_blocks:>6} {t['valu']:>6} {t['scalar']:>6} {t['lds']:>5} {t['vmem']:>5} "
            f"{t['save']:>6} {t['restore']:>7} {t['data_rd']:>7}")


HEAD = f"{'':<46} {'blocks':>6} {'VALU':>6} {'scalar':>6} {'LDS':>5} {'VMEM':>5} {'saves':>6} {'restores':>7} {'data rd':>7}"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="assembly text (hipcc -S --offload-device-only)")
    ap.add_argument("kernel", help="a substring of the kernel's symbol, e.g. k_scan_skipILb0ELi8E")
    ap.add_argument("--candidate-loop", help="label of the candidate loop's header instead of the automatic choice")
    ap.add_argument("--all-blocks", action="store_true", help="list every block, not only those with spill moves")
    ap.add_argument("--blocks", help="comma-separated block names: print the sum over this path as well")
    args = ap.parse_args()

    sym, lines = kernel_lines(args.asm, args.kernel)
    blocks = parse(lines)
    spill = find_spill_vgprs(blocks)
    classify(blocks, spill)
    loops, reachable = loops_of(blocks)
    idx = {b.name: i for i, b in enumerate(blocks)}

    headers = sorted(loops, key=lambda h: (len(loops[h]), h), reverse=True)
    parent: dict[int, int | None] = {}
    for h in loops:  # the smallest loop that contains this one
        outer = [g for g in loops if g != h and h in loops[g] and loops[h] <= loops[g]]
        parent[h] = min(outer, key=lambda g: len(loops[g])) if outer else None
    depth_of_loop = {}
    for h in loops:
        d, g = 1, parent[h]
        while g is not None:
            d, g = d + 1, parent[g]
        depth_of_loop[h] = d
    inner: dict[int, int | None] = {}  # block -> header of its innermost loop
    for i in range(len(blocks)):
        inside = [h for h in loops if i in loops[h]]
        inner[i] = min(inside, key=lambda h: len(loops[h])) if inside else None

    print(f"kernel   {sym}")
    everything = total(blocks, range(len(blocks)))
    print(f"blocks   {len(blocks)} ({len(reachable)} reachable from the entry), loops {len(loops)}")
    print(f"spill VGPRs (v_writelane_b32 destinations no other instruction names): "
          f"{', '.join('v%d' % r for r in sorted(spill)) or 'none'}")
    print(f"static   VALU {everything['valu']}  scalar {everything['scalar']}  LDS {everything['lds']}  VMEM {everything['vmem']}")
    print(f"         spill saves {everything['save']}  spill restores {everything['restore']}  "
          f"data lane reads {everything['data_rd']}  data lane writes {sum(b.data_wr for b in blocks)}")
    print()

    # ---- the candidate loop
    cand = None
    if args.candidate_loop:
        if args.candidate_loop not in idx or idx[args.candidate_loop] not in loops:
            sys.exit(f"{args.candidate_loop} is not a loop header of this kernel")
        cand = idx[args.candidate_loop]
    else:
        second = [h for h in loops if depth_of_loop[h] == 2]
        if second:
            cand = max(second, key=lambda h: (total(blocks, loops[h])["data_rd"], len(loops[h])))
    region = ["" for _ in blocks]
    if cand is not None and parent[cand] is not None:
        chunk = parent[cand]
        c_lo, c_hi = min(loops[cand]), max(loops[cand])
        k_lo, k_hi = min(loops[chunk]), max(loops[chunk])
        merge = [h for h in loops if parent[h] == cand]
        merge_h = max(merge, key=lambda h: len(loops[h])) if merge else None
        for i in range(len(blocks)):
            if i in loops[cand]:
                if inner[i] == cand:
                    region[i] = "cand: per tile"
                elif merge_h is not None and inner[i] == merge_h:
                    region[i] = "cand: per tile and merge"
                elif merge_h is not None and i in loops[merge_h]:
                    region[i] = "cand: loops inside a merge's turn"
                else:
                    region[i] = "cand: other inner loops"
            elif i in loops[chunk]:
                region[i] = "sweep (chunk loop, in front)" if i < c_lo else "chunk end (behind the candidate loop)"
            elif i < k_lo:
                region[i] = "entry, roles, riders (in front of the chunk loop)"
            else:
                region[i] = "flush, ticket, selection (behind the chunk loop)"
        print(f"candidate loop: header {blocks[cand].name} (line {blocks[cand].line}), {len(loops[cand])} blocks, layout "
              f"{blocks[c_lo].name} .. {blocks[c_hi].name}")
        print(f"chunk loop:     header {blocks[chunk].name} (line {blocks[chunk].line}), {len(loops[chunk])} blocks, layout "
              f"{blocks[k_lo].name} .. {blocks[k_hi].name}")
        if merge_h is not None:
            print(f"merge loop:     header {blocks[merge_h].name} (line {blocks[merge_h].line}), {len(loops[merge_h])} blocks")
        print()
        print("By region (static counts; a block that is laid out behind the chunk loop but belongs to it counts with the loop)")
        print(HEAD)
        order = ["entry, roles, riders (in front of the chunk loop)", "sweep (chunk loop, in front)", "cand: per tile",
                 "cand: per tile and merge", "cand: loops inside a merge's turn", "cand: other inner loops",
                 "chunk end (behind the candidate loop)", "flush, ticket, selection (behind the chunk loop)"]
        for name in order:
            members = [i for i, r in enumerate(region) if r == name]
            if members:
                print(row(name, len(members), total(blocks, members)))
        print()
    else:
        print("candidate loop: not found (no loop nested inside another one)\n")

    print("Loops (counts include nested loops)")
    print(HEAD)
    for h in sorted(loops, key=lambda h: min(loops[h])):
        tag = " <- candidate loop" if h == cand else ""
        label = f"{'  ' * (depth_of_loop[h] - 1)}{blocks[h].name} depth {depth_of_loop[h]}{tag}"
        print(row(label, len(loops[h]), total(blocks, loops[h])))
    print()

    print("Blocks" + ("" if args.all_blocks else " with spill moves") + " (depth = loops around the block)")
    print(f"{'block':<14} {'line':>7} {'depth':>5} {'VALU':>5} {'scalar':>6} {'LDS':>4} {'VMEM':>4} {'saves':>5} {'restores':>8} {'data rd':>7}  region")
    for i, b in enumerate(blocks):
        if not args.all_blocks and not (b.save or b.restore):
            continue
        d = depth_of_loop[inner[i]] if inner[i] is not None else 0
        print(f"{b.name:<14} {b.line:>7} {d:>5} {b.valu:>5} {b.scalar:>6} {b.lds:>4} {b.vmem:>4} {b.save:>5} {b.restore:>8} {b.data_rd:>7}  {region[i]}")

    if args.blocks:
        names = [x.strip() for x in args.blocks.split(",") if x.strip()]
        missing = [x for x in names if x not in idx]
        if missing:
            sys.exit(f"no such block: {', '.join(missing)}")
        print()
        print(HEAD)
        print(row("path " + " ".join(names)[:40], len(names), total(blocks, [idx[x] for x in names])))


if __name__ == "__main__":
    main()
