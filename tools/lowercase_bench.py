#!/usr/bin/env python3
"""Dev tool: what yabpe_lowercase (str.lower() on the device) costs.  Text resident in HBM, the call timed on the
host around it (it ends in a synchronise; allocation included, as in normalize_bench.py) for 7 repetitions after a warm-up, with
the phase times of yabpe_lowercase_stats of the fastest repetition.  yabpe_pretokenize with the GPT-2 pattern (split_pattern 0)
runs in turn with it inside every repetition on the same text: the yardstick every row is a ratio to.  A device-to-device copy
of the same number of bytes (torch's Tensor.copy_, device events) is timed once per size: what the device copies at.
   python tools/lowercase_bench.py [--mib 256,1024] [--text lower,caps,mixed,cyrgreek,sigma,resize,capsigma] [--reps 7]
Texts: `lower` = ASCII words, already lower case (path 0); `caps` = ASCII words over an alphabet with capitals (path 1); `mixed`
= the multilingual lexicon text of group_bench.py (its path is reported); `cyrgreek` = Cyrillic and Greek in capitals without a
sigma (path 1); `sigma` = Greek in capitals with sigmas, final ones among them (path 2); `resize` = a text dense in U+212A and
U+0130 (path 2); `capsigma` = `caps` with one capital sigma in the middle (path 2 on text that is ASCII but for two bytes).  Run
every text at two sizes and compare the time per byte: the call must stay linear.  Prints one JSON line
per text and size, one for the pre-tokeniser on it, and one per size for the copy."""
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
ap.add_argument("--mib", default="256,1024")
ap.add_argument("--text", default="lower,caps,mixed,cyrgreek,sigma,resize,capsigma")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
SP = ["<|endoftext|>"]

UNITS = {
    "cyrgreek": "\u041f\u0420\u0418\u0412\u0415\u0422 \u041c\u0418\u0420, \u039a\u0391\u039b\u0397\u039c\u0395\u03a1\u0391 \u039a\u039f\u039c\u0397 \u0416\u0418\u0417\u041d\u042c\n".encode(),
    "sigma": "\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 \u039a\u0391\u0399 \u039f\u0399 \u03a3\u03a5\u039d\u03a4\u03a1\u039f\u03a6\u039f\u0399 \u03a4\u039f\u03a5\u03a3, \u03a3'\u0391\u0393\u0391\u03a0\u03a9\n".encode(),
    "resize": "\u212a\u0130 \u212aelvin \u0130stanbul \u023a\u023e x\n".encode(),
}


def fill(ctx, n: int, unit: bytes) -> tuple[int, int]:
    """About n bytes of `unit` repeated on the device, whole units only: written in pieces over a generated buffer of that size"""
    pb, _po, _nw, nb = ctx.synth_generate(n, 1_000, 3, b"ab", False)
    nb -= nb % len(unit)
    piece = np.frombuffer(unit * max(1, min(nb, 64 << 20) // len(unit)), np.uint8)
    for a in range(0, nb, len(piece)):
        ctx.h2d(pb + a, piece[:min(len(piece), nb - a)])
    return pb, nb


def copy_rate(n: int, reps: int):
    """min ms of a device-to-device copy of n bytes (n read, n written), or None when torch is not there"""
    try:
        import torch
    except ImportError:
        return None
    a = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    ms = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return min(ms)


for mib in [int(x) for x in args.mib.split(",")]:
    cms = copy_rate(mib << 20, args.reps)
    print(json.dumps({"label": args.label, "call": "device copy (torch Tensor.copy_)", "mib": mib, "min_ms": None if cms is None else round(cms, 3),
                      "gb_per_s_read_plus_written": None if cms is None else round(2 * (mib << 20) / cms / 1e6, 1)}), flush=True)
    for kind in args.text.split(","):
        with _native.Context() as ctx:
            if kind == "lower":
                pb, _po, _nw, nb = ctx.synth_generate(mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyz", True)
            elif kind == "caps":
                pb, _po, _nw, nb = ctx.synth_generate(mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLM", True)
            elif kind == "capsigma":  # (one sigma sends the whole call down path 2: what ASCII pays there)
                pb, _po, _nw, nb = ctx.synth_generate(mib << 20, 50_000, 2, b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLM", True)
                ctx.h2d(pb + nb // 2, np.frombuffer(b"\xce\xa3", np.uint8))
            elif kind == "mixed":
                lex, off = synth.text_lexicon(20_000, 5)
                pb, _po, _nw, nb = ctx.synth_generate_lex(mib << 20, 5, lex, off)
            elif kind in UNITS:
                pb, nb = fill(ctx, mib << 20, UNITS[kind])
            else:
                raise SystemExit(f"unknown text {kind!r}")
            ms, pre_ms, best = [], [], None
            for rep in range(args.reps + 1):  # (the first repetition warms up: code objects, the table, the allocator's cache)
                t0 = time.perf_counter()
                ctx.lowercase(pb, n_bytes=nb)
                dt = (time.perf_counter() - t0) * 1e3
                st = ctx.lowercase_stats()
                ctx.lowercase_free()
                if rep:
                    ms.append(dt)
                    if dt == min(ms):
                        best = st
                t0 = time.perf_counter()
                ctx.pretokenize(pb, n_bytes=nb, special_tokens=SP)
                dt = (time.perf_counter() - t0) * 1e3
                ctx.pretokenize_free()
                if rep:
                    pre_ms.append(dt)
            row = {"label": args.label, "text": kind, "call": "lowercase", "mib": round(nb / 2**20, 1), "path": best["path"], "min_ms": round(min(ms), 2),
                   "median_ms": round(statistics.median(ms), 2), "max_ms": round(max(ms), 2), "gb_per_s": round(nb / min(ms) / 1e6, 1),
                   "ns_per_kib": round(min(ms) * 1e6 / (nb / 1024), 2), "ratio_to_pretokenize": round(min(ms) / min(pre_ms), 3),
                   "copies_worth_of_time": None if cms is None else round(min(ms) / (cms * nb / (mib << 20)), 2),
                   **{k: best[k] for k in ("n_bytes_out", "n_changed", "n_resized", "n_sigma", "n_final_sigma", "n_copied")},
                   **{k: round(best[k], 2) for k in ("check_ms", "scan_ms", "write_ms", "total_ms")}}
            print(json.dumps(row), flush=True)
            print(json.dumps({"label": args.label, "text": kind, "call": "pretokenize (split_pattern 0)", "mib": round(nb / 2**20, 1), "min_ms": round(min(pre_ms), 2),
                              "median_ms": round(statistics.median(pre_ms), 2), "max_ms": round(max(pre_ms), 2), "gb_per_s": round(nb / min(pre_ms) / 1e6, 1),
                              "ns_per_kib": round(min(pre_ms) * 1e6 / (nb / 1024), 2)}), flush=True)
