#!/usr/bin/env python3
"""Dev tool: what the digit-group pass (option "digit_group") costs the device pre-tokeniser.  Synthetic text
resident in HBM, yabpe_pretokenize timed on the host around the call (it ends in a synchronise; allocation included, as in
pretok_bench.py), every group in turn inside every repetition so that drift hits them alike.
   python tools/group_bench.py [--mib 1024] [--digit-group 0,3] [--text words,mixed,digits] [--reps 7]
Texts: `words` = pretok_bench.py's (space + lower-case word, no digit at all), `mixed` = synth.text_lexicon (8% numbers of
1..6 digits, multi-byte scripts, punctuation, whitespace runs), `digits` = nothing but ASCII digits, one run -- the case the
pass must stay linear on.  YABPE_LIB=<another libyabpe.so> measures another build (one that does not know the option runs
the GPT-2 path whatever the group).  Prints one JSON line per (text, group)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
from yet_another_bpe import _native, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--digit-group", default="0,3")
ap.add_argument("--text", default="words,mixed,digits")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
groups = [int(g) for g in args.digit_group.split(",")]
SP = ["<|endoftext|>"]

for kind in args.text.split(","):
    with _native.Context() as ctx:
        if kind == "words":
            pb, _po, _nw, nb = ctx.synth_generate(args.mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyz", True)
        elif kind == "digits":
            pb, _po, _nw, nb = ctx.synth_generate(args.mib << 20, 1_000, 3, b"0123456789", False)
        elif kind == "mixed":
            lex, off = synth.text_lexicon(20_000, 5)
            pb, _po, _nw, nb = ctx.synth_generate_lex(args.mib << 20, 5, lex, off)
        else:
            raise SystemExit(f"unknown text {kind!r}")
        ms = {g: [] for g in groups}
        words = {}
        for rep in range(args.reps + 1):  # (the first repetition warms up: code objects, the allocator's cache)
            for g in groups:
                ctx.set_option("digit_group", g)
                t0 = time.perf_counter()
                _dt, _do, n_words = ctx.pretokenize(pb, n_bytes=nb, special_tokens=SP)
                dt = time.perf_counter() - t0
                ctx.pretokenize_free()
                words[g] = n_words
                if rep:
                    ms[g].append(dt * 1e3)
        base = min(ms[groups[0]])
        for g in groups:
            print(json.dumps({"label": args.label, "text": kind, "mib": round(nb / 2**20, 1), "digit_group": g, "pretokens": words[g],
                              "min_ms": round(min(ms[g]), 2), "median_ms": round(statistics.median(ms[g]), 2), "max_ms": round(max(ms[g]), 2),
                              "gb_per_s": round(nb / min(ms[g]) / 1e6, 1), f"ratio_to_group_{groups[0]}": round(min(ms[g]) / base, 3)}), flush=True)
