#!/usr/bin/env python3
"""Dev tool: the device encoder (yabpe_encode) on 1 GiB of synth.text_lexicon text generated on the device, with a
32,000-merge model trained on the device from that text; device time per phase from yabpe_encode_stats after a warm-up,
GB/s of text and ids/s.  For comparison, the plain-Python BBPETokenizer.encode (one core) on a 16 MiB sample of the text.
--offsets byte|char: also yabpe_encode_spans (ids plus every id's span in that unit) in the same run, its per-phase times
printed next to the plain call's.
   python tools/encode_bench.py [--mib 1024] [--merges 32000] [--reps 3] [--py-mib 16] [--offsets byte|char] [--json out.json]"""
import argparse, json, sys, time
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
from yet_another_bpe import _native, synth
from yet_another_bpe.tokenizer import BBPETokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--merges", type=int, default=32000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--py-mib", type=int, default=16)
ap.add_argument("--offsets", choices=["byte", "char"], default="")
ap.add_argument("--json", default="")
a = ap.parse_args()

lb, lo = synth.text_lexicon(30000, 11)
with _native.Context() as gen:
    tb, _to, _np, tn = gen.synth_generate_lex(a.mib << 20, 11, lb, lo)
    dt, do, nw = gen.pretokenize(tb, n_bytes=tn)
    base = [bytes([b]) for b in range(256)]
    with _native.Context() as tr:
        tr.set_vocab(base)
        tr.load_words_ptr(dt, do, nw, dedup=True)
        left, right, merged, _c = tr.train(a.merges, 1)
    gen.pretokenize_free()
    toks, merges = list(base), []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        merges.append((toks[l], toks[r]))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
    vocab = {t: i for i, t in enumerate(toks)}
    gen.encode_set_model(vocab, merges, [], 0)
    def timed(call):
        call()  # warm-up
        out = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall = time.perf_counter() - t0
            st = gen.encode_stats()
            st["wall_ms"] = 1e3 * wall
            out.append(st)
        return out

    runs = timed(lambda: gen.encode(tb, n_bytes=tn))
    span_runs = timed(lambda: gen.encode_spans(tb, n_bytes=tn, chars=a.offsets == "char")) if a.offsets else []
    sample = gen.d2h(tb, min(tn, a.py_mib << 20)).tobytes()
while sample and sample[-1] & 0xC0 == 0x80 or (sample and sample[-1] >= 0xC0):
    sample = sample[:-1]
text = sample.decode("utf-8")
tok = BBPETokenizer(vocab=vocab, merges=merges)
t0 = time.perf_counter()
py_ids = tok.encode(text)
py_s = time.perf_counter() - t0
best = min(runs, key=lambda r: r["total_ms"])
phases = ("split_ms", "pretok_ms", "pool_ms", "words_ms", "emit_ms")
out = {"text_bytes": tn, "merges": len(merges), "pretokens": best["n_pretokens"], "unique_words": best["n_unique"],
       "unique_long": best["n_unique_long"], "ids": best["n_ids"], **{k: round(best[k], 3) for k in phases},
       "device_total_ms": round(best["total_ms"], 3), "phase_sum_ms": round(sum(best[k] for k in phases), 3),
       "call_wall_ms": round(best["wall_ms"], 3), "GB_per_s_device": round(tn / best["total_ms"] / 1e6, 2),
       "ids_per_s_device": round(best["n_ids"] / best["total_ms"] * 1e3), "all_total_ms": [round(r["total_ms"], 3) for r in runs],
       "python_one_core": {"text_bytes": len(sample), "seconds": round(py_s, 3), "MB_per_s": round(len(sample) / py_s / 1e6, 3),
                           "ids_per_s": round(len(py_ids) / py_s)}}
if span_runs:
    sb = min(span_runs, key=lambda r: r["total_ms"])
    out["offsets"] = {"unit": a.offsets, **{k: round(sb[k], 3) for k in phases}, "device_total_ms": round(sb["total_ms"], 3),
                      "call_wall_ms": round(sb["wall_ms"], 3), "GB_per_s_device": round(tn / sb["total_ms"] / 1e6, 2),
                      "all_total_ms": [round(r["total_ms"], 3) for r in span_runs],
                      "total_vs_plain": round(sb["total_ms"] / best["total_ms"], 3)}
    print(f"{'phase':<10}{'plain ms':>12}{'spans(' + a.offsets + ') ms':>18}", file=sys.stderr)
    for k in phases + ("total_ms",):
        print(f"{k[:-3]:<10}{best[k]:>12.3f}{sb[k]:>18.3f}", file=sys.stderr)
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
