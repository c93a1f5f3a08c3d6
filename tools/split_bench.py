#!/usr/bin/env python3
"""Dev tool: what the cl100k and the o200k_base split pattern (option "split_pattern" = 1 and 3) cost the
device pre-tokeniser against the GPT-2 pattern with the same digit group.  Synthetic text resident in HBM, yabpe_pretokenize timed on the host around the
call (it ends in a synchronise; allocation included, as in group_bench.py), every variant in turn inside every repetition so
that drift hits them alike.
   python tools/split_bench.py [--mib 1024] [--pattern 0,1,3] [--digit-group 3] [--text words,mixed,blank,nlspaces] [--reps 7]
Texts: `words` and `mixed` as in group_bench.py; `blank` = nothing but U+000A (a file of blank lines: one pre-token, every
byte inside one newline run); `nlspaces` = one U+000A and then nothing but spaces (every byte behind the first waits for the
backward scan).  The last two are the cases the newline pass must stay linear on: run them at two sizes and compare the time
per byte.  The chains of the o200k_base scanner, likewise: `kana` = nothing but U+30A2 (one word of \\p{Lo}), `camel` = "A" U+30A2
repeated (upper case and \\p{Lo} in turn: one word), `upper` = nothing but "A", `bang` = nothing but "!", `contr` = "'s" repeated
behind a letter, `nlslash` = U+000A "/" repeated behind a "!".  YABPE_LIB=<another libyabpe.so> measures another build with --pattern 0.  Prints one JSON line per (text, pattern)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
from yet_another_bpe import _native, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--pattern", default="0,1")
ap.add_argument("--digit-group", type=int, default=3)
ap.add_argument("--text", default="words,mixed,blank,nlspaces")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
patterns = [int(p) for p in args.pattern.split(",")]
SP = ["<|endoftext|>"]


def fill(ctx, n: int, unit, first: int) -> tuple[int, int]:
    """About n bytes of `unit` (a byte value or bytes) repeated on the device, whole units only, the first byte `first`: written in
    pieces over a generated buffer of that size"""
    unit = bytes([unit]) if isinstance(unit, int) else unit
    pb, _po, _nw, nb = ctx.synth_generate(n, 1_000, 3, b"ab", False)
    nb -= nb % len(unit)
    piece = np.frombuffer(unit * (min(nb, 64 << 20) // len(unit)), np.uint8)
    for a in range(0, nb, len(piece)):
        ctx.h2d(pb + a, piece[:min(len(piece), nb - a)])
    ctx.h2d(pb, np.array([first], np.uint8))
    return pb, nb


CHAINS = {"kana": ("ア".encode(), 0xE3), "camel": ("Aア".encode(), 0x41), "upper": (b"A", 0x41), "bang": (b"!", 0x21), "contr": (b"'s", 0x61), "nlslash": (b"\n/", 0x21)}


for kind in args.text.split(","):
    with _native.Context() as ctx:
        if kind == "words":
            pb, _po, _nw, nb = ctx.synth_generate(args.mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyz", True)
        elif kind == "mixed":
            lex, off = synth.text_lexicon(20_000, 5)
            pb, _po, _nw, nb = ctx.synth_generate_lex(args.mib << 20, 5, lex, off)
        elif kind == "blank":
            pb, nb = fill(ctx, args.mib << 20, 0x0A, 0x0A)
        elif kind == "nlspaces":
            pb, nb = fill(ctx, args.mib << 20, 0x20, 0x0A)
        elif kind in CHAINS:
            pb, nb = fill(ctx, args.mib << 20, *CHAINS[kind])
        else:
            raise SystemExit(f"unknown text {kind!r}")
        ms = {p: [] for p in patterns}
        words = {}
        for rep in range(args.reps + 1):  # (the first repetition warms up: code objects, the allocator's cache)
            for p in patterns:
                ctx.set_option("digit_group", args.digit_group)
                ctx.set_option("split_pattern", p)
                t0 = time.perf_counter()
                _dt, _do, n_words = ctx.pretokenize(pb, n_bytes=nb, special_tokens=SP)
                dt = time.perf_counter() - t0
                ctx.pretokenize_free()
                words[p] = n_words
                if rep:
                    ms[p].append(dt * 1e3)
        base = min(ms[patterns[0]])
        for p in patterns:
            print(json.dumps({"label": args.label, "text": kind, "mib": round(nb / 2**20, 1), "split_pattern": p, "digit_group": args.digit_group,
                              "pretokens": words[p], "min_ms": round(min(ms[p]), 2), "median_ms": round(statistics.median(ms[p]), 2),
                              "max_ms": round(max(ms[p]), 2), "gb_per_s": round(nb / min(ms[p]) / 1e6, 1), "ns_per_kib": round(min(ms[p]) * 1e6 / (nb / 1024), 2),
                              f"ratio_to_pattern_{patterns[0]}": round(min(ms[p]) / base, 3)}), flush=True)
