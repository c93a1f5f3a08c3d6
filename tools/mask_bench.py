#!/usr/bin/env python3
"""Dev tool: the masked-language-model calls (yabpe_encode_words, yabpe_mask) on synth.text_lexicon text generated on the
device, encoded with a model trained on the device from that text; documents cut at pre-token boundaries to a mean of about
--doc-ids ids.  Best of --reps after a warm-up, all in one run:
  * yabpe_encode_words total_ms and emit_ms against yabpe_encode's on the same text, alternating, and their ratios (the extra
    work: every document's first pre-token, and one u32 store per id in the emit pass);
  * yabpe_mask's mask_ms -- with words (whole-word masking: 8 B read and 8 B written per id) and without (4 B read, 8 B
    written) -- against a device-to-device hipMemcpyAsync of the same byte volume (HIP events), as GB/s and as a factor;
  * the counters of the draw at p = 0.15, 80 / 10 / 10.
   python tools/mask_bench.py [--mib 256] [--merges 8000] [--reps 3] [--doc-ids 1000] [--json out.json]"""
import argparse, ctypes, json, sys
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--doc-ids", type=int, default=1000)
ap.add_argument("--json", default="")
a = ap.parse_args()
T = BBPETokenizer._dropout_threshold


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
    # ---- yabpe_encode against yabpe_encode_words, alternating
    gen.encode(tb, n_bytes=tn, doc_starts=starts)  # warm-up
    gen.encode_words(tb, n_bytes=tn, doc_starts=starts)
    plain, words = [], []
    for _ in range(a.reps):
        gen.encode(tb, n_bytes=tn, doc_starts=starts)
        plain.append(gen.encode_stats())
        di, dd, dw, ni = gen.encode_words(tb, n_bytes=tn, doc_starts=starts)
        words.append(gen.encode_stats())
    bp, bw = min(plain, key=lambda s: s["total_ms"]), min(words, key=lambda s: s["total_ms"])
    out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "docs": n_docs, "mean_ids_per_doc": round(ni / n_docs, 1),
           "encode": {"total_ms": round(bp["total_ms"], 3), "emit_ms": round(bp["emit_ms"], 3), "all_total_ms": [round(s["total_ms"], 3) for s in plain]},
           "encode_words": {"total_ms": round(bw["total_ms"], 3), "emit_ms": round(bw["emit_ms"], 3),
                            "all_total_ms": [round(s["total_ms"], 3) for s in words]},
           "encode_words_total_vs_encode": round(bw["total_ms"] / bp["total_ms"], 4),
           "encode_words_emit_vs_encode": round(min(s["emit_ms"] for s in words) / min(s["emit_ms"] for s in plain), 4)}
    # ---- yabpe_mask on the device results, against a copy of the same byte volume
    rule = dict(seed=1, select=T(0.15), mask=T(0.8), random=T(0.1), mask_id=len(vocab), n_random=len(vocab))
    for name, w, whole, moved in (("mask_whole_word", dw, True, 16 * ni), ("mask_tokens_no_words", None, False, 12 * ni)):
        runs = []
        for k in range(a.reps + 1):
            gen.mask(di, ni, dd, n_docs, w, whole_word=whole, **rule)
            if k:
                runs.append(gen.mask_stats())
        st = min(runs, key=lambda s: s["mask_ms"])
        cp = copy_ms(moved // 2, a.reps)  # (a copy of B bytes moves 2 B)
        out[name] = {"mask_ms": round(st["mask_ms"], 4), "total_ms": round(st["total_ms"], 4), "all_mask_ms": [round(s["mask_ms"], 4) for s in runs],
                     "bytes_moved": moved, "GB_per_s": round(moved / st["mask_ms"] / 1e6, 1), "copy_same_bytes_ms": round(cp, 4),
                     "copy_GB_per_s": round(moved / cp / 1e6, 1), "mask_ms_vs_copy_ms": round(st["mask_ms"] / cp, 3),
                     "counters": {k: st[k] for k in ("n_protected", "n_selected", "n_masked", "n_random", "n_kept")},
                     "selected_share": round(st["n_selected"] / max(1, ni), 5)}
    gen.mask_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
