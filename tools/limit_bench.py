#!/usr/bin/env python3
"""Dev tool: what a maximum token length (option max_token_bytes) costs or saves.  The 256 MiB job of bench.py's
generator (synth.SynthSpec.config3: 256-value alphabet, 1M Zipf types, seed 3; flat layout, min_frequency 1) without a limit
and with limits 16 and 8: a dropped delta costs extra loads where a key would have entered the table, against a table that
holds fewer keys.  One warm-up job, then one timed job per setting; one JSON line per setting.  Not a gate.
   python tools/limit_bench.py [--mib 256] [--merges 32000] [--limits 0,16,8] [--verify]"""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
from yet_another_bpe import _native, synth

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--merges", type=int, default=32000)
ap.add_argument("--limits", default="0,16,8", help="comma-separated; 0 = no limit")
ap.add_argument("--verify", action="store_true", help="compare the table with a recount after every job (not part of the timing)")
a = ap.parse_args()
BASE = [bytes([b]) for b in range(256)] + [b"<|endoftext|>"]


def job(gen_ptrs, limit):
    pb, po, n_words = gen_ptrs
    with _native.Context() as ctx:
        ctx.set_option("max_token_bytes", limit)
        ctx.set_vocab(BASE)
        t0 = time.perf_counter()
        ctx.load_words_ptr(pb, po, n_words, dedup=False)
        left, right, merged, _count = ctx.train(a.merges, 1)
        wall = time.perf_counter() - t0
        st = ctx.stats()
        mism = ctx.verify_table() if a.verify else None
        lens = [len(t) for t in BASE]
        for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
            if m == len(lens):
                lens.append(lens[l] + lens[r])
    out = {"max_token_bytes": limit, "merges": len(left), "merges_per_s": round(len(left) / wall, 1), "wall_ms": round(wall * 1e3, 1),
           "load_ms": round(st["load_ms"], 1), "train_ms": round(st["train_ms"], 1), "table_entries": st["table_entries"],
           "table_capacity": st["table_capacity"], "table_rebuilds": st["table_rebuilds"],
           "launches": st["dense_launches"] + st["sparse_launches"],
           "longest_token": max(lens[len(BASE):], default=0), "tokens_final": st["tokens_now"]}
    if mism is not None:
        out["verify_mismatches"] = mism
    return out


spec = synth.SynthSpec.config3(a.mib << 20)
with _native.Context() as gen:
    pb, po, n_words, n_bytes = gen.synth_generate(spec.target_bytes, spec.n_types, spec.seed, spec.alphabet, spec.space_prefix)
    print(f"corpus on device: {n_bytes} bytes, {n_words} words", file=sys.stderr)
    job((pb, po, n_words), 0)  # warm-up: code objects, the block cache
    for limit in [int(x) for x in a.limits.split(",")]:
        print(json.dumps(job((pb, po, n_words), limit)), flush=True)
