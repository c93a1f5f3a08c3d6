#!/usr/bin/env python3
"""Dev tool: yabpe_span_corrupt on synth.text_lexicon text generated on the device, encoded with a model trained on the
device from that text; documents cut at pre-token boundaries to a mean of about --doc-ids ids.  Best of --reps after a
warm-up, timed with HIP events, all in one run on the same ids:
  * yabpe_span_corrupt's kernel_ms and its four phases (flags, run index, positions, write) at p = 0.15, mean 3, Lmax 10 --
    per word (words read) and per token without words -- against
  * yabpe_mask's mask_ms on the same ids,
  * a device-to-device hipMemcpyAsync of the bytes the call must read plus write (ids, words, both outputs: what a fused
    single pass would move; the passes' temporaries are not in this figure), and
  * the total_ms of the yabpe_encode_words call in front of it;
  * the counters of the draw.
   python tools/span_bench.py [--mib 256] [--merges 8000] [--reps 3] [--doc-ids 1000] [--json out.json]"""
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
PHASES = ("flags_ms", "index_ms", "place_ms", "write_ms")


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
    # ---- the call in front: yabpe_encode_words
    enc = []
    for k in range(a.reps + 1):
        di, dd, dw, ni = gen.encode_words(tb, n_bytes=tn, doc_starts=starts)
        if k:
            enc.append(gen.encode_stats())
    be = min(enc, key=lambda s: s["total_ms"])
    out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "docs": n_docs, "mean_ids_per_doc": round(ni / n_docs, 1),
           "encode_words": {"total_ms": round(be["total_ms"], 3), "all_total_ms": [round(s["total_ms"], 3) for s in enc]}}
    # ---- yabpe_mask on the same ids
    rule = dict(seed=1, select=T(0.15), mask=T(0.8), random=T(0.1), mask_id=len(vocab), n_random=len(vocab))
    for name, w, whole in (("mask_whole_word", dw, True), ("mask_tokens_no_words", None, False)):
        runs = []
        for k in range(a.reps + 1):
            gen.mask(di, ni, dd, n_docs, w, whole_word=whole, **rule)
            if k:
                runs.append(gen.mask_stats())
        out[name] = {"mask_ms": round(min(s["mask_ms"] for s in runs), 4), "all_mask_ms": [round(s["mask_ms"], 4) for s in runs]}
    gen.mask_free()
    # ---- yabpe_span_corrupt
    To, C = BBPETokenizer.span_thresholds(0.15, 3.0, 10)
    sent = np.arange(len(vocab), len(vocab) + 100, dtype=np.uint32)
    for name, w, whole, mask_name in (("span_whole_word", dw, True, "mask_whole_word"), ("span_tokens_no_words", None, False, "mask_tokens_no_words")):
        runs = []
        for k in range(a.reps + 1):
            gen.span_corrupt(di, ni, dd, n_docs, w, sentinels=sent, seed=1, open=To, lens=C, whole_word=whole, final_sentinel=True)
            if k:
                runs.append(gen.span_stats())
        st = min(runs, key=lambda s: s["kernel_ms"])
        moved = 4 * ni * (2 if w is not None else 1) + 4 * (st["n_in"] + st["n_tgt"])
        cp = copy_ms(moved // 2, a.reps)  # (a copy of B bytes moves 2 B)
        out[name] = {"kernel_ms": round(st["kernel_ms"], 4), "total_ms": round(st["total_ms"], 4), "all_kernel_ms": [round(s["kernel_ms"], 4) for s in runs],
                     **{p: round(st[p], 4) for p in PHASES}, "bytes_read_plus_written": moved, "GB_per_s": round(moved / st["kernel_ms"] / 1e6, 1),
                     "copy_same_bytes_ms": round(cp, 4), "copy_GB_per_s": round(moved / cp / 1e6, 1), "kernel_ms_vs_copy_ms": round(st["kernel_ms"] / cp, 3),
                     "kernel_ms_vs_mask_ms": round(st["kernel_ms"] / out[mask_name]["mask_ms"], 3),
                     "kernel_ms_vs_encode_words_total_ms": round(st["kernel_ms"] / be["total_ms"], 4),
                     "counters": {k: st[k] for k in ("n_protected", "n_noise", "n_runs", "n_runs_over", "n_cut", "n_in", "n_tgt")},
                     "noise_share": round(st["n_noise"] / max(1, ni), 5), "mean_run": round(st["n_noise"] / max(1, st["n_runs"]), 3)}
    gen.span_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
