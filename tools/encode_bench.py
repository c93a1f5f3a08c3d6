#!/usr/bin/env python3
"""Dev tool: the device encoder (yabpe_encode) on 1 GiB of synth.text_lexicon text generated on the device, with a
32,000-merge model trained on the device from that text; device time per phase from yabpe_encode_stats after a warm-up,
GB/s of text and ids/s.  For comparison, the plain-Python BBPETokenizer.encode (one core) on a 16 MiB sample of the text.
--offsets byte|char: also yabpe_encode_spans (ids plus every id's span in that unit) in the same run, its per-phase times
printed next to the plain call's.
--dropout P: also yabpe_encode_dropout at that probability in the same run -- its per-phase times next to the pooled call's,
its ratio to it, the same call with one wave per word (option dropout_pack = 0), the device memory the first such call takes
from the runtime, and the plain-Python encode_dropout on the sample.
   python tools/encode_bench.py [--mib 1024] [--merges 32000] [--reps 3] [--py-mib 16] [--offsets byte|char] [--dropout P]
                                [--json out.json]"""
import argparse, ctypes, json, sys, time
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
ap.add_argument("--dropout", type=float, default=None)
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

    def device_free() -> int:
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        ctypes.CDLL("libamdhip64.so").hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
        return free.value

    drop_runs, wave_runs, drop_mem = [], [], 0
    if a.dropout is not None:  # (first: what its first call takes from the runtime is measured before any other encode)
        T = BBPETokenizer._dropout_threshold(a.dropout)
        gen.encode_free()
        free0 = device_free()
        gen.encode_dropout(tb, T, 1, n_bytes=tn)
        drop_mem = free0 - device_free()
        drop_runs = timed(lambda: gen.encode_dropout(tb, T, 1, n_bytes=tn))
        gen.set_option("dropout_pack", 0)
        wave_runs = timed(lambda: gen.encode_dropout(tb, T, 1, n_bytes=tn))
        gen.set_option("dropout_pack", 1)
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
if drop_runs:
    db, wb = min(drop_runs, key=lambda r: r["total_ms"]), min(wave_runs, key=lambda r: r["total_ms"])
    t0 = time.perf_counter()
    py_drop = tok.encode_dropout(text, a.dropout, 1)
    pyd_s = time.perf_counter() - t0
    dev_ids_s = db["n_ids"] / db["total_ms"] * 1e3
    out["dropout"] = {"p": a.dropout, "ids": db["n_ids"], "long_words": db["n_unique_long"], **{k: round(db[k], 3) for k in phases},
                      "device_total_ms": round(db["total_ms"], 3), "call_wall_ms": round(db["wall_ms"], 3),
                      "GB_per_s_device": round(tn / db["total_ms"] / 1e6, 2), "ids_per_s_device": round(dev_ids_s),
                      "all_total_ms": [round(r["total_ms"], 3) for r in drop_runs], "total_vs_pooled": round(db["total_ms"] / best["total_ms"], 3),
                      "one_wave_per_word": {"words_ms": round(wb["words_ms"], 3), "emit_ms": round(wb["emit_ms"], 3),
                                            "device_total_ms": round(wb["total_ms"], 3), "all_total_ms": [round(r["total_ms"], 3) for r in wave_runs],
                                            "total_vs_packed": round(wb["total_ms"] / db["total_ms"], 3)},
                      "first_call_device_bytes": drop_mem,
                      "python_one_core": {"text_bytes": len(sample), "seconds": round(pyd_s, 3), "ids_per_s": round(len(py_drop) / pyd_s),
                                          "device_vs_python_ids_per_s": round(dev_ids_s / (len(py_drop) / pyd_s), 1)}}
    print(f"{'phase':<10}{'pooled ms':>12}{'dropout ms':>14}{'one wave/word ms':>20}", file=sys.stderr)
    for k in phases + ("total_ms",):
        print(f"{k[:-3]:<10}{best[k]:>12.3f}{db[k]:>14.3f}{wb[k]:>20.3f}", file=sys.stderr)
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
