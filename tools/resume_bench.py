#!/usr/bin/env python3
"""Dev tool: what continuing from a saved model costs against what a user paid before (training those merges again).
On synth.text_lexicon text generated on the device, pooled layout: a from-scratch job trains N merges (train_ms: device
time of yabpe_train); a fresh context then loads the same words resumed at those N merges (segment_ms: pooling + replay of
every unique word, build_ms: tiles + initial pair count, from yabpe_resume_stats) and both train K more merges, which must
agree.  The load_ms of the from-scratch job is reported too (both jobs pay a load).
   python tools/resume_bench.py [--mib 256] [--merges 10000] [--more 200] [--reps 3] [--json out.json]"""
import argparse, json, sys
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth
from yet_another_bpe.trainer import BBPETrainer

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--merges", type=int, default=10000)
ap.add_argument("--more", type=int, default=200)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default="")
a = ap.parse_args()

lb, lo = synth.text_lexicon(30000, 11)
base = [bytes([b]) for b in range(256)]
with _native.Context() as gen:
    tb, _to, _np, tn = gen.synth_generate_lex(a.mib << 20, 11, lb, lo)
    dt, do, nw = gen.pretokenize(tb, n_bytes=tn)
    with _native.Context() as tr:
        tr.set_vocab(base)
        tr.load_words_ptr(dt, do, nw, dedup=True)
        left, right, merged, _c = tr.train(a.merges, 1)
        scratch = tr.stats()
        checksum = tr.stream_checksum()
        more = tr.train(a.more, 1)
    vocab, merges = BBPETrainer._decode_merges(base, left, right, merged)
    toks, triples = _native.merge_triples(base, merges)
    runs = []
    for _ in range(a.reps + 1):  # (the first one warms up)
        with _native.Context() as rs:
            rs.set_vocab(toks)
            rs.load_words_resumed_ptr(dt, do, nw, triples, dedup=True)
            st = rs.resume_stats()
            assert rs.stream_checksum() == checksum, "resumed state differs from the trained one"
            again = rs.train(a.more, 1)
            assert all(np.array_equal(x, y) for x, y in zip(more, again)), "continued merges differ"
        runs.append(st)
best = min(runs[1:], key=lambda r: r["segment_ms"] + r["build_ms"])
resumed_ms = best["segment_ms"] + best["build_ms"]
out = {"text_bytes": tn, "pretokens": nw, "unique_words": best["n_unique"], "merges": len(merges),
       "tokens_after_replay": best["tokens"], "long_words_after_replay": best["n_long"],
       "segment_ms": round(best["segment_ms"], 3), "build_ms": round(best["build_ms"], 3), "resumed_load_ms": round(resumed_ms, 3),
       "scratch_load_ms": round(scratch["load_ms"], 3), "scratch_train_ms": round(scratch["train_ms"], 3),
       "train_over_resumed_load": round(scratch["train_ms"] / resumed_ms, 2),
       "all_resumed_load_ms": [round(r["segment_ms"] + r["build_ms"], 3) for r in runs[1:]]}
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
