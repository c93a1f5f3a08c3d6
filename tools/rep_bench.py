#!/usr/bin/env python3
"""Dev tool: repetition signals (yabpe_repetition), HIP events inside the call, medians of --reps runs after a warm-up, the
three cases alternating in one run, on the corpus of tools/dup_bench.py (synth.text_lexicon text generated, trained on and
encoded on the device, documents of about --doc-ids ids; the device pointers of yabpe_encode passed straight in) at the nine
default lengths 2 .. 10:
  (a) short   the call as it is: documents of at most REP_DOC ids counted in LDS, every length from one read;
  (b) long    the same call with the option rep_doc_max = 1: every document through the table in HBM, once per length;
  (c) dup     yabpe_dup_spans at min_len = --dup-len on the same ids, the yardstick of existing code; the line also holds nine
              times its median, what nine such passes would cost.
Per case: the medians of the call's parts and of its total, and ids x lengths per second; the results of (a) and (b) must be
equal.  Then the plain-Python rule (BBPETokenizer.repetition_stats) on one host core over the first --host-docs documents,
checked against the device's result for those documents value for value.
   python tools/rep_bench.py [--mib 256] [--reps 7] [--out profiles/rep_bench.txt]"""
import argparse, json, statistics, sys, time
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth
from yet_another_bpe.tokenizer import BBPETokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--merges", type=int, default=8000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--doc-ids", type=int, default=1000)
ap.add_argument("--dup-len", type=int, default=5)
ap.add_argument("--host-docs", type=int, default=300)
ap.add_argument("--out", default="")
a = ap.parse_args()
NGRAMS = BBPETokenizer.REP_NGRAMS
lines = []


def emit(out):
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)


def median_stats(runs):
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0] if k.endswith("_ms")}


# text -> ids on the device, as tools/dup_bench.py
lb, lo = synth.text_lexicon(30000, 11)
with _native.Context() as gen:
    tb, _to, _np, tn = gen.synth_generate_lex(a.mib << 20, 11, lb, lo)
    dt, do, nw = gen.pretokenize(tb, n_bytes=tn)
    pre_off = gen.d2h(do, 8 * (nw + 1), np.uint64)
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
    gen.encode_set_model({t: i for i, t in enumerate(toks)}, merges, [], 0)
    _di, _dd, n_all = gen.encode(tb, n_bytes=tn)
    text_starts = np.ascontiguousarray(pre_off[:-1:max(1, round(a.doc_ids * nw / n_all))])
    di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=text_starts)
    nd = len(text_starts)
    same_run = {"text_bytes": tn, "encode_total_ms": round(gen.encode_stats()["total_ms"], 3)}

    def rep(doc_max):
        gen.set_option("rep_doc_max", doc_max)
        try:
            ptrs = gen.repetition(di, ni, dd, nd, ngrams=NGRAMS)
        finally:
            gen.set_option("rep_doc_max", 0)
        return ptrs, gen.repetition_stats()

    runs = {"short": [], "long": [], "dup": []}
    results = {}
    for k in range(a.reps + 1):  # (the first round is the warm-up; the cases alternate)
        for name, doc_max in (("short", 0), ("long", 1)):
            ptrs, st = rep(doc_max)
            if k:
                runs[name].append(st)
            else:
                results[name] = [gen.d2h(p, 4 * nd * len(NGRAMS), np.uint32) for p in ptrs[:3]]
        gen.dup_spans(di, ni, dd, nd, min_len=a.dup_len)
        if k:
            runs["dup"].append(gen.dup_spans_stats())
    equal = all(np.array_equal(x, y) for x, y in zip(results["short"], results["long"]))
    med = {name: median_stats(r) for name, r in runs.items()}
    for name in ("short", "long"):
        st = runs[name][0]
        emit({"case": name, "ngrams": list(NGRAMS), **{k: v for k, v in st.items() if not k.endswith("_ms")}, **med[name],
              "all_total_ms": [round(r["total_ms"], 4) for r in runs[name]],
              "G_id_lengths_per_s": round(ni * len(NGRAMS) / max(med[name]["total_ms"], 1e-9) / 1e6, 2), **same_run})
    st = runs["dup"][0]
    emit({"case": "dup", "min_len": a.dup_len, "n_windows": st["n_windows"], "n_slots": st["n_slots"], **med["dup"],
          "all_total_ms": [round(r["total_ms"], 4) for r in runs["dup"]], "nine_times_total_ms": round(9 * med["dup"]["total_ms"], 4)})
    emit({"case": "summary", "short_equals_long": bool(equal), "long_over_short": round(med["long"]["total_ms"] / max(med["short"]["total_ms"], 1e-9), 2),
          "nine_dup_over_short": round(9 * med["dup"]["total_ms"] / max(med["short"]["total_ms"], 1e-9), 2),
          "nine_dup_over_long": round(9 * med["dup"]["total_ms"] / max(med["long"]["total_ms"], 1e-9), 2)})
    # the host rule over a sample, against the device on the same sample
    hd = min(a.host_docs, nd)
    starts = gen.d2h(dd, 8 * (nd + 1), np.uint64)
    ids = gen.d2h(di, 4 * int(starts[hd]), np.uint32)
    docs = [ids[int(starts[d]):int(starts[d + 1])].tolist() for d in range(hd)]
    t0 = time.perf_counter()
    exp = BBPETokenizer().repetition_stats(docs, ngrams=NGRAMS)
    host_s = time.perf_counter() - t0
    got = gen.repetition_to_host(ids, None, starts[:hd], None, ngrams=NGRAMS)
    emit({"case": "host rule", "docs": hd, "ids": len(ids), "seconds": round(host_s, 3), "device_total_ms": round(gen.repetition_stats()["total_ms"], 4),
          "equals_device": bool(all(g.tolist() == e for g, e in zip(got, exp)))})
    gen.repetition_free()
    gen.dup_spans_free()
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
