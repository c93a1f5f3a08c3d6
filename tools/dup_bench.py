#!/usr/bin/env python3
"""Dev tool: exact-substring duplicates (yabpe_dup_spans), HIP events inside the call, best of --reps after a warm-up, all in
one run, on the corpus of tools/cluster_bench.py (synth.text_lexicon text generated, trained on and encoded on the device,
documents of about --doc-ids ids) at min_len = --min-len with YABPE_DUP_COMPACT:
  (a) the corpus as it is, the device pointers of yabpe_encode passed straight in;
  (b) the same ids with a --planted share of the documents carrying one of --paragraphs paragraphs of --para-ids ids,
      copied from the corpus over the document's own ids (host arrays; the staging copy lies in front of the first event);
  (c) an all-identical corpus: the first document's ids in every document.
Per case: plan / insert / mark / compact / total ms, windows per second of the insert and of the call, the same-run floor
(tools/cluster_floor: one random 4-byte atomicMin per window into a table of the same size) and insert_ms over it, and the
plain-Python rule (BBPETokenizer.duplicate_spans) on one host core over the first --host-docs documents, checked against the
device's result for those documents mask for mask and statistic for statistic.
   python tools/dup_bench.py [--mib 256] [--reps 5] [--min-len 50] [--out profiles/dup_bench.txt]"""
import argparse, json, subprocess, sys, time
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--doc-ids", type=int, default=1000)
ap.add_argument("--min-len", type=int, default=50)
ap.add_argument("--planted", type=float, default=0.2)
ap.add_argument("--paragraphs", type=int, default=100)
ap.add_argument("--para-ids", type=int, default=200)
ap.add_argument("--host-docs", type=int, default=300)
ap.add_argument("--out", default="")
a = ap.parse_args()
N = a.min_len
TOK = BBPETokenizer()
floor_bin = REPO / "tools" / "cluster_floor"
if not floor_bin.exists():
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", str(floor_bin), str(REPO / "tools" / "cluster_floor.hip")])
lines = []


def case(ctx, name, ids, n_ids, starts, n_docs, extra=None):
    """One measured case: ids / starts host arrays or device pointers."""
    runs = []
    for k in range(a.reps + 1):  # (the first one is the warm-up)
        ctx.dup_spans(ids, n_ids, starts, n_docs, min_len=N, compact=True)
        if k:
            runs.append(ctx.dup_spans_stats())
    st = min(runs, key=lambda s: s["total_ms"])
    lg = st["n_slots"].bit_length() - 1
    floor = json.loads(subprocess.check_output([str(floor_bin), str(lg), str(max(st["n_windows"], 1)), str(a.reps)], timeout=300))
    out = {"case": name, "min_len": N, **{k: v for k, v in st.items() if not k.endswith("_ms")},
           **{k: round(st[k], 4) for k in ("plan_ms", "insert_ms", "mark_ms", "compact_ms", "total_ms")},
           "all_insert_ms": [round(s["insert_ms"], 4) for s in runs], "M_windows_per_s_insert": round(st["n_windows"] / max(st["insert_ms"], 1e-9) / 1e3, 1),
           "M_windows_per_s_call": round(st["n_windows"] / max(st["total_ms"], 1e-9) / 1e3, 1),
           "floor_atomic_min_ms": floor["atomic_min_ms"], "insert_over_floor": round(st["insert_ms"] / max(floor["atomic_min_ms"], 1e-9), 2)}
    if isinstance(ids, np.ndarray):  # the host rule over a sample, against the device on the same sample
        hd = min(a.host_docs, len(starts))
        end = int(starts[hd]) if hd < len(starts) else len(ids)
        docs = [ids[int(starts[d]):(int(starts[d + 1]) if d + 1 < hd else end)].tolist() for d in range(hd)]
        t0 = time.perf_counter()
        masks, n_dup, exp_st = TOK.duplicate_spans(docs, min_len=N)
        host_s = time.perf_counter() - t0
        dup, got_n, _k, _o = ctx.dup_spans_to_host(ids[:end], None, starts[:hd], None, min_len=N)
        dst = ctx.dup_spans_stats()
        out["host_rule"] = {"docs": hd, "ids": end, "seconds": round(host_s, 3), "device_total_ms": round(dst["total_ms"], 4),
                            "equals_device": bool(dup.tolist() == [m for mk in masks for m in mk] and got_n.tolist() == n_dup
                                                  and all(dst[k] == v for k, v in exp_st.items()))}
    out.update(extra or {})
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)


# text -> ids on the device, as tools/cluster_bench.py
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
    case(gen, "corpus, device pointers of yabpe_encode", di, ni, dd, nd, same_run)
    ids = gen.d2h(di, 4 * ni, np.uint32)
    starts = gen.d2h(dd, 8 * nd, np.uint64)
    case(gen, "corpus, host arrays", ids, None, starts, None, same_run)
    # (b) repeated paragraphs: one of a few paragraphs over the own ids of a share of the documents
    rng = np.random.default_rng(5)
    lens = np.diff(np.append(starts, np.uint64(ni))).astype(np.int64)
    planted = ids.copy()
    paras = [ids[s:s + a.para_ids].copy() for s in rng.integers(0, ni - a.para_ids, a.paragraphs)]
    hit = np.flatnonzero((rng.random(nd) < a.planted) & (lens > a.para_ids))
    for d in hit.tolist():
        at = int(starts[d]) + int(rng.integers(0, lens[d] - a.para_ids + 1))
        planted[at:at + a.para_ids] = paras[int(rng.integers(0, a.paragraphs))]
    case(gen, f"corpus, {len(hit)} documents ({a.planted:.0%}) with one of {a.paragraphs} paragraphs of {a.para_ids} ids", planted, None, starts, None, same_run)
    # (c) one document for everybody
    doc = ids[:int(lens[0])]
    n_same = max(1, ni // len(doc))
    case(gen, f"identical, {n_same} documents of {len(doc)} ids", np.tile(doc, n_same), None, (np.arange(n_same, dtype=np.uint64) * np.uint64(len(doc))), None)
    gen.dup_spans_free()
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
