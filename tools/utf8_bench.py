#!/usr/bin/env python3
"""Dev tool: what yabpe_utf8_repair (errors="replace" / "ignore" on the device) costs.  Text resident in HBM, the
call timed on the host around it (it ends in a synchronise; allocation included, as in normalize_bench.py), with the pass times
of yabpe_utf8_repair_stats of the fastest repetition.  On the valid texts yabpe_pretokenize with the GPT-2 pattern runs in turn
with it inside every repetition: the yardstick the valid path is compared with.
   python tools/utf8_bench.py [--mib 256] [--text words,mixed,damaged,stray] [--mode replace,ignore] [--reps 7]
Texts: `words` and `mixed` as in group_bench.py (valid: the call stops after the check pass); `damaged` = `words` with a seeded
1 % of the bytes replaced by a byte >= 0x80 of tests/decode_helpers.CLASS_BYTES; `stray` = nothing but 0x80 (3 x the bytes out
under "replace", none under "ignore").  Run the last two at two sizes and compare the time per byte: the pass must stay linear.
Prints one JSON line per text and mode (and one for the pre-tokeniser on the valid texts)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
from yet_another_bpe import _native, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--text", default="words,mixed,damaged,stray")
ap.add_argument("--mode", default="replace,ignore")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
SP = ["<|endoftext|>"]
HIGH = np.array([0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF], np.uint8)
PIECE = 64 << 20


def words(ctx) -> tuple[int, int]:
    pb, _po, _nw, nb = ctx.synth_generate(args.mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyz", True)
    return pb, nb


def damage(ctx, pb: int, nb: int) -> None:
    """1 % of the bytes (drawn with replacement), seeded, piece by piece through the host"""
    rng = np.random.default_rng(7)
    for a in range(0, nb, PIECE):
        piece = ctx.d2h(pb + a, min(PIECE, nb - a))
        at = rng.integers(0, len(piece), len(piece) // 100)
        piece[at] = HIGH[rng.integers(0, len(HIGH), len(at))]
        ctx.h2d(pb + a, piece)


def stray(ctx, pb: int, nb: int) -> None:
    piece = np.full(min(nb, PIECE), 0x80, np.uint8)
    for a in range(0, nb, len(piece)):
        ctx.h2d(pb + a, piece[:min(len(piece), nb - a)])


for kind in args.text.split(","):
    with _native.Context() as ctx:
        if kind in ("words", "damaged", "stray"):
            pb, nb = words(ctx)
            if kind != "words":
                (damage if kind == "damaged" else stray)(ctx, pb, nb)
        elif kind == "mixed":
            lex, off = synth.text_lexicon(20_000, 5)
            pb, _po, _nw, nb = ctx.synth_generate_lex(args.mib << 20, 5, lex, off)
        else:
            raise SystemExit(f"unknown text {kind!r}")
        valid = kind in ("words", "mixed")
        for mode in args.mode.split(","):
            ms, pre_ms, best = [], [], None
            for rep in range(args.reps + 1):  # (the first repetition warms up: code objects, the allocator's cache)
                t0 = time.perf_counter()
                ctx.utf8_repair(pb, n_bytes=nb, mode=_native.UTF8_MODES[mode])
                dt = (time.perf_counter() - t0) * 1e3
                st = ctx.utf8_repair_stats()
                ctx.utf8_repair_free()
                if rep:
                    ms.append(dt)
                    if dt == min(ms):
                        best = st
                if valid:
                    t0 = time.perf_counter()
                    ctx.pretokenize(pb, n_bytes=nb, special_tokens=SP)
                    dt = (time.perf_counter() - t0) * 1e3
                    ctx.pretokenize_free()
                    if rep:
                        pre_ms.append(dt)
            row = {"label": args.label, "text": kind, "call": f"utf8_repair ({mode})", "mib": round(nb / 2**20, 1), "min_ms": round(min(ms), 2),
                   "median_ms": round(statistics.median(ms), 2), "max_ms": round(max(ms), 2), "gb_per_s": round(nb / min(ms) / 1e6, 1),
                   "ns_per_kib": round(min(ms) * 1e6 / (nb / 1024), 2), **{k: best[k] for k in ("n_bytes_out", "n_subparts", "first_bad_pos")},
                   **{k: round(best[k], 2) for k in ("check_ms", "write_ms", "total_ms")}}
            if valid:
                row["ratio_to_pretokenize"] = round(min(ms) / min(pre_ms), 3)
            print(json.dumps(row), flush=True)
            if valid:
                print(json.dumps({"label": args.label, "text": kind, "call": "pretokenize (split_pattern 0)", "mib": round(nb / 2**20, 1),
                                  "min_ms": round(min(pre_ms), 2), "median_ms": round(statistics.median(pre_ms), 2), "max_ms": round(max(pre_ms), 2),
                                  "gb_per_s": round(nb / min(pre_ms) / 1e6, 1), "ns_per_kib": round(min(pre_ms) * 1e6 / (nb / 1024), 2)}), flush=True)
