#!/usr/bin/env python3
"""Dev tool: what yabpe_normalize (NFC on the device) costs.  Text resident in HBM, the call timed on the host
around it (it ends in a synchronise; allocation included, as in split_bench.py), with the phase times of yabpe_normalize_stats
of the fastest repetition.  On the clean texts yabpe_pretokenize with the GPT-2 pattern runs in turn with it inside every
repetition: the yardstick the clean path is compared with.
   python tools/normalize_bench.py [--mib 256] [--text words,mixed,nfd,marks,jamo,yesmarks] [--reps 7]
Texts: `words` and `mixed` as in group_bench.py (clean: the call stops after the class pass); `nfd` = the multilingual text of
the split tests in NFD, repeated (dirty throughout); `marks` = "a" and 30 times U+0301, repeated (one dirty segment of 31 code
points each); `jamo` = U+1100 U+1161 U+11A8 repeated (every syllable composed from three); `yesmarks` = nothing but U+0591 (ccc
220, quick-check Yes: ONE clean segment as long as the text).  Run the last three at two sizes and compare the time per byte:
the normaliser must stay linear on them.  Prints one JSON line per text (and one for the pre-tokeniser on the clean texts)."""
import argparse
import json
import statistics
import sys
import time
import unicodedata
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
from yet_another_bpe import _native, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--text", default="words,mixed,nfd,marks,jamo,yesmarks")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
SP = ["<|endoftext|>"]


def fill(ctx, n: int, unit: bytes) -> tuple[int, int]:
    """About n bytes of `unit` repeated on the device, whole units only: written in pieces over a generated buffer of that size"""
    pb, _po, _nw, nb = ctx.synth_generate(n, 1_000, 3, b"ab", False)
    nb -= nb % len(unit)
    piece = np.frombuffer(unit * max(1, min(nb, 64 << 20) // len(unit)), np.uint8)
    for a in range(0, nb, len(piece)):
        ctx.h2d(pb + a, piece[:min(len(piece), nb - a)])
    return pb, nb


def nfd_unit() -> bytes:
    from tests import split5_helpers as sh

    return unicodedata.normalize("NFD", sh.multilingual(REPO / "tests" / "golden").decode("utf-8") + "\n").encode("utf-8")


UNITS = {"marks": lambda: ("a" + "\u0301" * 30).encode(), "jamo": lambda: "\u1100\u1161\u11a8".encode(), "yesmarks": lambda: "\u0591".encode(), "nfd": nfd_unit}

for kind in args.text.split(","):
    with _native.Context() as ctx:
        if kind == "words":
            pb, _po, _nw, nb = ctx.synth_generate(args.mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyz", True)
        elif kind == "mixed":
            lex, off = synth.text_lexicon(20_000, 5)
            pb, _po, _nw, nb = ctx.synth_generate_lex(args.mib << 20, 5, lex, off)
        elif kind in UNITS:
            pb, nb = fill(ctx, args.mib << 20, UNITS[kind]())
        else:
            raise SystemExit(f"unknown text {kind!r}")
        clean = kind in ("words", "mixed")
        ms, pre_ms, best = [], [], None
        for rep in range(args.reps + 1):  # (the first repetition warms up: code objects, the tables, the allocator's cache)
            t0 = time.perf_counter()
            ctx.normalize(pb, n_bytes=nb)
            dt = (time.perf_counter() - t0) * 1e3
            st = ctx.normalize_stats()
            ctx.normalize_free()
            if rep:
                ms.append(dt)
                if dt == min(ms):
                    best = st
            if clean:
                t0 = time.perf_counter()
                ctx.pretokenize(pb, n_bytes=nb, special_tokens=SP)
                dt = (time.perf_counter() - t0) * 1e3
                ctx.pretokenize_free()
                if rep:
                    pre_ms.append(dt)
        row = {"label": args.label, "text": kind, "call": "normalize", "mib": round(nb / 2**20, 1), "min_ms": round(min(ms), 2), "median_ms": round(statistics.median(ms), 2),
               "max_ms": round(max(ms), 2), "gb_per_s": round(nb / min(ms) / 1e6, 1), "ns_per_kib": round(min(ms) * 1e6 / (nb / 1024), 2),
               **{k: best[k] for k in ("n_bytes_out", "n_suspects", "n_dirty", "n_dirty_long", "n_copied")},
               **{k: round(best[k], 2) for k in ("class_ms", "find_ms", "segments_ms", "write_ms", "total_ms")}}
        if clean:
            row["ratio_to_pretokenize"] = round(min(ms) / min(pre_ms), 3)
        print(json.dumps(row), flush=True)
        if clean:
            print(json.dumps({"label": args.label, "text": kind, "call": "pretokenize (split_pattern 0)", "mib": round(nb / 2**20, 1), "min_ms": round(min(pre_ms), 2),
                              "median_ms": round(statistics.median(pre_ms), 2), "max_ms": round(max(pre_ms), 2), "gb_per_s": round(nb / min(pre_ms) / 1e6, 1),
                              "ns_per_kib": round(min(pre_ms) * 1e6 / (nb / 1024), 2)}), flush=True)
