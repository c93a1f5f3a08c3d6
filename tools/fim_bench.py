#!/usr/bin/env python3
"""Dev tool: the fill-in-the-middle calls on synth.text_lexicon text generated on the device, encoded with a model trained on
the device from that text; documents cut at pre-token boundaries to a mean of about --doc-ids ids (the text and the model of
tools/mask_bench.py and tools/span_bench.py).  Best of --reps after a warm-up, timed with HIP events, all in one run:
  * yabpe_fim at token level (fim_rate 0.5, spm_rate 0.5, eot, no cut): plan_ms, write_ms and their sum,
  * yabpe_fim_cuts on the text: cuts_ms,
  * yabpe_fim with pieces on the ids of the 3 n pieces,
  * the total_ms of yabpe_encode over the 3 n pieces against yabpe_encode over the n documents,
  * per call a device-to-device hipMemcpyAsync of the bytes it must read plus write (ids in, ids and labels out; for the
    cuts the text in and 48 bytes a document out; the per-document plan is not in this figure),
  * the counters of the draw.
   python tools/fim_bench.py [--mib 256] [--merges 8000] [--reps 3] [--doc-ids 1000] [--json out.json]"""
import argparse, ctypes, json, sys
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--merges", type=int, default=8000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--doc-ids", type=int, default=1000)
ap.add_argument("--json", default="")
a = ap.parse_args()


def copy_ms(n_bytes: int, reps: int) -> float:
    """best device time of hipMemcpyAsync(device to device) of n_bytes, HIP events on the null stream"""
    hip = ctypes.CDLL("libamdhip64.so")
    src, dst, e0, e1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float(0)
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(n_bytes))); ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(n_bytes)))
    ok(hip.hipMemset(src, 1, ctypes.c_size_t(n_bytes))); ok(hip.hipEventCreate(ctypes.byref(e0))); ok(hip.hipEventCreate(ctypes.byref(e1)))
    best = float("inf")
    for k in range(reps + 1):  # (the first one is the warm-up)
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(n_bytes), 3, None))
        ok(hip.hipEventRecord(e1, None)); ok(hip.hipEventSynchronize(e1)); ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        best = min(best, ms.value) if k else best
    hip.hipFree(src); hip.hipFree(dst); hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return best


def against_copy(ms: float, moved: int) -> dict:
    cp = copy_ms(moved // 2, a.reps)  # (a copy of B bytes moves 2 B)
    return {"bytes_read_plus_written": moved, "GB_per_s": round(moved / ms / 1e6, 1), "copy_same_bytes_ms": round(cp, 4),
            "copy_GB_per_s": round(moved / cp / 1e6, 1), "ms_vs_copy_ms": round(ms / cp, 3)}


COUNTERS = ("n_docs", "n_psm", "n_spm", "n_truncated_docs", "n_ids_dropped", "n_out")
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
    vocab = {t: i for i, t in enumerate(toks)}
    gen.encode_set_model(vocab, merges, [], 0)
    _di, _dd, n_all = gen.encode(tb, n_bytes=tn)
    step = max(1, round(a.doc_ids * nw / n_all))  # pre-tokens per document
    starts = np.ascontiguousarray(pre_off[:-1:step])
    n_docs = len(starts)
    V = len(vocab)
    rule = dict(seed=1, fim=1 << 31, spm=1 << 31, pre_id=V, suf_id=V + 1, mid_id=V + 2, eot_id=V + 3)
    # ---- the cuts on the text (the lead-byte table, the draws, the selects)
    runs = []
    for k in range(a.reps + 1):
        dpo, dcu, _nd = gen.fim_cuts(tb, tn, starts, seed=1, fim=1 << 31, spm=1 << 31)
        if k:
            runs.append(gen.fim_stats()["cuts_ms"])
    out = {"text_bytes": tn, "merges": len(merges), "docs": n_docs}
    out["fim_cuts"] = {"cuts_ms": round(min(runs), 4), "all_cuts_ms": [round(x, 4) for x in runs], **against_copy(min(runs), tn + 48 * n_docs)}
    piece_off = gen.d2h(dpo, 24 * n_docs, np.uint64)
    # ---- yabpe_encode over the 3 n pieces, then yabpe_fim with pieces on its ids
    enc3 = []
    for k in range(a.reps + 1):
        di3, dd3, ni3 = gen.encode(tb, n_bytes=tn, doc_starts=piece_off)
        if k:
            enc3.append(gen.encode_stats()["total_ms"])

    def fim_runs(name, di, ni, dd, nd, cuts, **kw):
        runs = []
        for k in range(a.reps + 1):
            gen.fim(di, ni, dd, nd, cuts, **rule, **kw)
            if k:
                runs.append(gen.fim_stats())
        st = min(runs, key=lambda s: s["plan_ms"] + s["write_ms"])
        ms = st["plan_ms"] + st["write_ms"]
        out[name] = {"ids": ni, "plan_plus_write_ms": round(ms, 4), "plan_ms": round(st["plan_ms"], 4), "write_ms": round(st["write_ms"], 4),
                     "total_ms": round(st["total_ms"], 4), "all_plan_plus_write_ms": [round(s["plan_ms"] + s["write_ms"], 4) for s in runs],
                     **against_copy(ms, 4 * ni + 8 * st["n_out"]), "counters": {c: st[c] for c in COUNTERS}}

    fim_runs("fim_pieces", di3, ni3, dd3, 3 * n_docs, dcu, pieces=True)
    # ---- yabpe_encode over the n documents, then yabpe_fim at token level on its ids
    enc1 = []
    for k in range(a.reps + 1):
        di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=starts)
        if k:
            enc1.append(gen.encode_stats()["total_ms"])
    fim_runs("fim_tokens", di, ni, dd, n_docs, None)
    out["mean_ids_per_doc"] = round(ni / n_docs, 1)
    out["encode"] = {"documents_total_ms": round(min(enc1), 3), "pieces_total_ms": round(min(enc3), 3), "pieces_vs_documents": round(min(enc3) / min(enc1), 4),
                     "ids_documents": ni, "ids_pieces": ni3, "all_documents_total_ms": [round(x, 3) for x in enc1], "all_pieces_total_ms": [round(x, 3) for x in enc3]}
    # ---- yabpe_mask on the same ids, for the neighbour's figure from this run
    runs = []
    for k in range(a.reps + 1):
        gen.mask(di, ni, dd, n_docs, None, seed=1, select=int(0.15 * 2**32), mask=int(0.8 * 2**32), random=int(0.1 * 2**32), mask_id=V, n_random=V)
        if k:
            runs.append(gen.mask_stats()["mask_ms"])
    out["mask_tokens_no_words"] = {"mask_ms": round(min(runs), 4), **against_copy(min(runs), 12 * ni)}
    gen.mask_free()
    gen.fim_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
