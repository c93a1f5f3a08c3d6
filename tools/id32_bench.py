#!/usr/bin/env python3
"""Dev tool: the two stages of a job past 65,534 tokens on bench.py's synthetic corpus, pooled: the u16 path to
65,534 tokens, the hand-over (resumed load with id_bits = 32: replay of every merge so far + tiles + initial count), then the
u32 path in ranges of 10,000 merges up to 100,000 and 200,000 tokens (or to where the corpus runs out of pairs, which is said).
For comparison the u16 path in the same regime: the same job with batch_max = 1 (one merge per launch), its last 5,000 merges
before 65,534 tokens.  Device times are HIP-event times (yabpe_stats train_ms, yabpe_resume_stats); the stream bytes per merge
are the live u32 slots + tile lengths a pass reads, as the driver counts them at its checks.
   python tools/id32_bench.py [--mib 1024] [--tokens 100000,200000] [--out profiles/id32_bench.txt]"""
import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
import numpy as np
from yet_another_bpe import _native, synth

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--tokens", default="100000,200000")
ap.add_argument("--out", default=str(REPO / "profiles" / "id32_bench.txt"))
a = ap.parse_args()
HBM_PEAK = 8.0e12  # bytes / s (bench.py's figure for the MI355X)
U16 = 65_534
BASE = [bytes([b]) for b in range(256)] + [b"<|endoftext|>"]
targets = sorted(int(x) for x in a.tokens.split(","))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


spec = synth.SynthSpec.config3(a.mib << 20)
with _native.Context() as gen:
    pb, po, nw, nb = gen.synth_generate(spec.target_bytes, spec.n_types, spec.seed, spec.alphabet, spec.space_prefix)
    say(f"corpus: {nb} bytes, {nw} words (bench.py's synthetic corpus, {a.mib} MiB), pooled on the device")
    # ---- stage 1 twice: as the trainer runs it, and with one merge per launch (the regime the u32 path is compared in)
    n1 = U16 - len(BASE)
    with _native.Context() as ctx:
        ctx.set_vocab(BASE)
        ctx.load_words_ptr(pb, po, nw, dedup=True)
        left, right, merged, _c = ctx.train(n1, 1)
        st = ctx.stats()
        say(f"u16 stage: {len(left)} merges in {st['train_ms'] / 1e3:.3f} s ({st['train_ms'] * 1e3 / max(1, len(left)):.1f} us per merge), "
            f"load {st['load_ms']:.1f} ms, {st['n_words']} unique words")
    with _native.Context() as ctx:
        ctx.set_option("batch_max", 1)
        ctx.set_vocab(BASE)
        ctx.load_words_ptr(pb, po, nw, dedup=True)
        ctx.train(len(left) - 5000, 1)
        t0 = ctx.stats()["train_ms"]
        tail = ctx.train(5000, 1)
        u16_tail_us = (ctx.stats()["train_ms"] - t0) * 1e3 / max(1, len(tail[0]))
        say(f"u16 path, batch_max = 1, its last {len(tail[0])} merges before {U16} tokens: {u16_tail_us:.1f} us per merge")
    toks, _merges = None, None
    vocab, merges_b = _native.decode_merges(BASE, left, right, merged)
    toks = sorted(vocab, key=vocab.get)
    say(f"tokens after the u16 stage: {len(toks)}")
    # ---- hand-over + stage 2
    with _native.Context() as ctx:
        ctx.set_option("id_bits", 32)
        ctx.set_vocab(toks)
        ctx.load_words_resumed_ptr(pb, po, nw, (left, right, merged), dedup=True)
        rs, st = ctx.resume_stats(), ctx.stats()
        say(f"hand-over: replay of {len(left)} merges + load {rs['segment_ms'] + rs['build_ms']:.1f} ms "
            f"(pooling + replay {rs['segment_ms']:.1f}, tiles + initial count {rs['build_ms']:.1f}); {rs['n_unique']} words, {rs['tokens']} tokens, "
            f"{st['n_tiles']} tiles, {rs['n_long']} long words")
        n_tok, total_ms, total_merges, first5000 = len(toks), 0.0, 0, None
        prev = ctx.stats()
        out_of_pairs = False
        first = ctx.train(5000, 1)
        cur = ctx.stats()
        first5000 = (cur["train_ms"] - prev["train_ms"]) * 1e3 / max(1, len(first[0]))
        say(f"u32 path, its first {len(first[0])} merges: {first5000:.1f} us per merge = {first5000 / u16_tail_us:.2f} x the u16 figure above")
        n_tok += len({int(m) for m in first[2].tolist() if m >= n_tok})
        total_ms += cur["train_ms"] - prev["train_ms"]
        total_merges += len(first[0])
        out_of_pairs = len(first[0]) < 5000
        prev = cur
        for target in targets:
            while n_tok < target and not out_of_pairs:
                ask = min(10_000, target - n_tok)
                got = ctx.train(ask, 1)
                cur = ctx.stats()
                ms = cur["train_ms"] - prev["train_ms"]
                nbytes = cur["dense_actual_bytes_sampled"] - prev["dense_actual_bytes_sampled"]
                k = max(1, len(got[0]))
                say(f"  u32 merges {total_merges:6d} .. {total_merges + len(got[0]):6d}: {ms * 1e3 / k:7.1f} us per merge, stream {nbytes / k / 1e6:6.2f} MB per merge, "
                    f"{nbytes / (ms / 1e3) / HBM_PEAK * 100 if ms else 0:5.2f} % of HBM peak over the whole time; table {cur['table_entries']} pairs / {cur['table_capacity']} slots, "
                    f"{cur['n_tiles']} tiles, {cur['retiles']} repacks")
                n_tok += len({int(m) for m in got[2].tolist() if m >= n_tok})
                total_ms += ms
                total_merges += len(got[0])
                out_of_pairs = len(got[0]) < ask
                prev = cur
            say(f"to {target} tokens: u32 stage {total_ms / 1e3:.3f} s for {total_merges} merges, {n_tok} tokens"
                + (" -- the corpus ran out of pairs here" if out_of_pairs else ""))
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
