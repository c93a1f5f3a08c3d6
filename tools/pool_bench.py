#!/usr/bin/env python3
"""Dev tool: text -> loaded merge loop through the word pool (batches: yabpe_pretokenize -> yabpe_pool_add, then
yabpe_pool_get -> yabpe_load_words) at several batch sizes, against the one-shot path (one yabpe_pretokenize, one
yabpe_load_words with YABPE_LOAD_DEDUP) on the same text.  The text is synth.text_lexicon text generated on the device (or a
file staged there once) and stays resident, so disk and host-to-device copies are in neither figure; the batches are slices of
it cut at the reference's chunk cuts.  Per batch size: a warm-up pass, then --reps passes; wall time of the whole pass (host
gaps included) and the device time of the phases (HIP events: yabpe_pool_stats, yabpe_stats).
   python tools/pool_bench.py [--mib 1024] [--batch-mib 64,256,1024] [--chunk-mib 8] [--reps 3] [--file PATH] [--json OUT]"""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
import numpy as np
from yet_another_bpe import _native, synth
from yet_another_bpe.trainer import chunk_ranges, group_chunks

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--batch-mib", default="64,256,1024")
ap.add_argument("--chunk-mib", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--file")
ap.add_argument("--json")
a = ap.parse_args()
SP = ["<|endoftext|>"]
BASE = [bytes([b]) for b in range(256)] + [s.encode() for s in SP]


def one_shot(ctx, text, n, starts):
    t0 = time.perf_counter()
    dt, do, nw = ctx.pretokenize(text, n_bytes=n, chunk_starts=starts, special_tokens=SP)
    t1 = time.perf_counter()
    ctx.load_words_ptr(dt, do, nw, dedup=True)
    ctx.pretokenize_free()
    t2 = time.perf_counter()
    st = ctx.stats()
    return {"wall_ms": (t2 - t0) * 1e3, "pretok_wall_ms": (t1 - t0) * 1e3, "load_ms": st["load_ms"], "n_words": nw, "n_unique": st["n_words"]}


def batched(ctx, text, ranges, batch_bytes):
    ev = {"pool_ms": 0.0, "probe_ms": 0.0, "append_ms": 0.0, "add_total_ms": 0.0}
    pretok = add = 0.0
    t0 = time.perf_counter()
    batches = group_chunks([b - a0 for a0, b in ranges], batch_bytes)
    for first, end in batches:
        lo, hi = ranges[first][0], ranges[end - 1][1]
        ta = time.perf_counter()
        dt, do, nw = ctx.pretokenize(text + lo, n_bytes=hi - lo, chunk_starts=[r[0] - lo for r in ranges[first:end]], special_tokens=SP)
        tb = time.perf_counter()
        ctx.pool_add_ptr(dt, do, nw)
        tc = time.perf_counter()
        ctx.pretokenize_free()
        pretok, add = pretok + (tb - ta), add + (tc - tb)
        ps = ctx.pool_stats()
        for k in ("pool_ms", "probe_ms", "append_ms"):
            ev[k] += ps[k]
        ev["add_total_ms"] += ps["total_ms"]
    pb, po, pf, nu, nb = ctx.pool_get()
    ps = ctx.pool_stats()
    t1 = time.perf_counter()
    ctx.load_words_ptr(pb, po, nu, freq_ptr=pf, dedup=False)
    ctx.pool_clear()
    t2 = time.perf_counter()
    return {"wall_ms": (t2 - t0) * 1e3, "pretok_wall_ms": pretok * 1e3, "add_wall_ms": add * 1e3, **ev, "load_ms": ctx.stats()["load_ms"],
            "load_wall_ms": (t2 - t1) * 1e3, "n_batches": len(batches), "n_unique": nu, "pool_bytes": nb,
            "slot_growths": ps["slot_growths"], "arena_growths": ps["arena_growths"]}


def best(runs):
    b = min(runs, key=lambda r: r["wall_ms"])
    return {**b, "wall_ms_all": [round(r["wall_ms"], 1) for r in runs]}


with _native.Context() as ctx:
    if a.file:
        data = np.fromfile(a.file, dtype=np.uint8)
        n = int(data.size)
        lb, lo_ = np.frombuffer(b"x", dtype=np.uint8), np.array([0, 1], dtype=np.uint64)
        text, _o, _p, _n = ctx.synth_generate_lex(n, 1, lb, lo_)  # (a device buffer of n bytes, then the file over it)
        ctx.h2d(text, data)
        del data
    else:
        lb, lo_ = synth.text_lexicon(30000, 11)
        text, _o, _p, n = ctx.synth_generate_lex(a.mib << 20, 11, lb, lo_)
    ranges = chunk_ranges(n, a.chunk_mib << 20, lambda off, k: ctx.d2h(text + off, k).tobytes())
    starts = [r[0] for r in ranges]
    assert all(x[1] == y[0] for x, y in zip(ranges[:-1], ranges[1:])), "a skipped byte between chunks: not handled by this tool"
    ctx.set_vocab(BASE)
    out = {"n_bytes": n, "n_chunks": len(ranges), "chunk_mib": a.chunk_mib, "reps": a.reps}
    one_shot(ctx, text, n, starts)  # warm-up (allocations land in the block cache)
    out["one_shot"] = best([one_shot(ctx, text, n, starts) for _ in range(a.reps)])
    ref = out["one_shot"]
    print(f"text {n / 2**20:.0f} MiB, {ref['n_words']} pre-tokens, {ref['n_unique']} unique; {len(ranges)} chunks of {a.chunk_mib} MiB")
    print(f"one-shot : text->loaded {ref['wall_ms']:8.1f} ms wall {ref['wall_ms_all']} = {n / ref['wall_ms'] / 1e6:.2f} GB/s"
          f"  (pretok {ref['pretok_wall_ms']:.1f} wall, load incl. pooling {ref['load_ms']:.1f} device)")
    out["batched"] = {}
    for mib in [int(x) for x in a.batch_mib.split(",")]:
        batched(ctx, text, ranges, mib << 20)
        r = best([batched(ctx, text, ranges, mib << 20) for _ in range(a.reps)])
        assert r["n_unique"] == ref["n_unique"], (r["n_unique"], ref["n_unique"])
        out["batched"][str(mib)] = r
        gbs = lambda ms: n / ms / 1e6 if ms else float("inf")  # noqa: E731
        print(f"batch {mib:5d} MiB x {r['n_batches']:3d}: text->loaded {r['wall_ms']:8.1f} ms wall {r['wall_ms_all']} = {gbs(r['wall_ms']):.2f} GB/s,"
              f" {r['wall_ms'] / ref['wall_ms']:.2f}x one-shot")
        print(f"    pretok {r['pretok_wall_ms']:.1f} wall ({gbs(r['pretok_wall_ms']):.1f} GB/s) | add {r['add_wall_ms']:.1f} wall: pool {r['pool_ms']:.1f}"
              f" ({gbs(r['pool_ms']):.1f} GB/s) probe {r['probe_ms']:.2f} append {r['append_ms']:.2f} device | load {r['load_ms']:.1f} device;"
              f" growths {r['slot_growths']} slots / {r['arena_growths']} arena; pool {r['pool_bytes'] / 2**20:.1f} MiB of words")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
