#!/usr/bin/env python3
"""Dev tool: yabpe_chat on synth.text_lexicon text generated on the device, encoded with a model trained on the device from
that text (the text and the model of tools/fim_bench.py); turns cut at pre-token boundaries to a mean of about --turn-ids
ids, --turns of them a conversation (system first, then user and assistant in turn), a template of 4-id headers and 2-id
footers with a 1-id prefix.  Best of --reps after a warm-up, timed with HIP events, all in one run:
  * yabpe_chat without a cut and with drop_oldest to --max-len: plan_ms, write_ms, total_ms,
  * per call a device-to-device hipMemcpyAsync of the bytes it must read plus write (content ids in, ids and labels out; the
    per-turn records are not in this figure),
  * yabpe_fim at token level with the conversations as documents (about the same number of output ids), and the write passes'
    time per output id against each other,
  * the counters of the call.
   python tools/chat_bench.py [--mib 256] [--merges 8000] [--reps 5] [--turn-ids 125] [--turns 8] [--max-len 512] [--json out.json]"""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--turn-ids", type=int, default=125)
ap.add_argument("--turns", type=int, default=8)
ap.add_argument("--max-len", type=int, default=512)
ap.add_argument("--json", default="")
a = ap.parse_args()


def copy_ms(n_bytes: int, reps: int) -> list:
    """device times of hipMemcpyAsync(device to device) of n_bytes after a warm-up, HIP events on the null stream"""
    hip = ctypes.CDLL("libamdhip64.so")
    src, dst, e0, e1, ms = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_float(0)
    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(n_bytes))); ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(n_bytes)))
    ok(hip.hipMemset(src, 1, ctypes.c_size_t(n_bytes))); ok(hip.hipEventCreate(ctypes.byref(e0))); ok(hip.hipEventCreate(ctypes.byref(e1)))
    runs = []
    for k in range(reps + 1):  # (the first one is the warm-up)
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(n_bytes), 3, None))
        ok(hip.hipEventRecord(e1, None)); ok(hip.hipEventSynchronize(e1)); ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        if k:
            runs.append(ms.value)
    hip.hipFree(src); hip.hipFree(dst); hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return runs


def spread(xs) -> dict:
    return {"min": round(min(xs), 4), "max": round(max(xs), 4), "all": [round(x, 4) for x in xs]}


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
    step = max(1, round(a.turn_ids * nw / n_all))  # pre-tokens per turn
    starts = np.ascontiguousarray(pre_off[:-1:step])
    n_turns = len(starts)
    di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=starts)  # every turn a document of its own
    conv_starts = np.arange(0, n_turns, a.turns, dtype=np.uint64)
    n_convs = len(conv_starts)
    roles = np.where(np.arange(n_turns) % a.turns == 0, 0, 1 + (np.arange(n_turns) % a.turns + 1) % 2).astype(np.uint8)  # system, user, assistant, ...
    V = len(vocab)
    tpl = dict(heads=[[V, V + 1 + r, V + 4, V + 5] for r in range(3)], feet=[[V + 6, V + 5]] * 3, prefix=[V + 7], train_mask=4, pin_mask=1)
    out = {"text_bytes": tn, "merges": len(merges), "turns": n_turns, "convs": n_convs, "content_ids": ni, "mean_ids_per_turn": round(ni / n_turns, 1)}
    COUNTERS = ("n_convs", "n_turns", "n_turns_dropped", "n_ids_cut", "n_out", "n_labelled", "n_convs_unlabelled")

    def chat_runs(name, **kw):
        runs = []
        for k in range(a.reps + 1):
            gen.chat(di, ni, dd, n_turns, conv_starts, None, roles, **tpl, **kw)
            if k:
                runs.append(gen.chat_stats())
        st = min(runs, key=lambda s: s["write_ms"])
        moved = 4 * (st["n_out"] if kw else ni) + 8 * st["n_out"]  # (with a cut only the kept contents must be read)
        cp = copy_ms(moved // 2, a.reps)  # (a copy of B bytes moves 2 B)
        out[name] = {"write_ms": spread([s["write_ms"] for s in runs]), "plan_ms": spread([s["plan_ms"] for s in runs]),
                     "total_ms": spread([s["total_ms"] for s in runs]), "bytes_read_plus_written": moved, "copy_same_bytes_ms": spread(cp),
                     "write_ms_vs_copy_ms": round(st["write_ms"] / min(cp), 3), "total_ms_vs_copy_ms": round(min(s["total_ms"] for s in runs) / min(cp), 3),
                     "write_ns_per_out_id": round(1e6 * st["write_ms"] / st["n_out"], 6), "counters": {c: st[c] for c in COUNTERS}}

    chat_runs("chat")
    chat_runs("chat_drop_oldest", max_len=a.max_len, drop_oldest=True, pin_first=True)
    # ---- yabpe_fim at token level, every conversation a document: about the same number of output ids
    conv_doc_starts = gen.d2h(dd, 8 * n_turns, np.uint64)[::a.turns].copy()
    runs = []
    for k in range(a.reps + 1):
        gen.fim(di, ni, conv_doc_starts, None, None, seed=1, fim=1 << 31, spm=1 << 31, pre_id=V, suf_id=V + 1, mid_id=V + 2, eot_id=V + 3)
        if k:
            runs.append(gen.fim_stats())
    st = min(runs, key=lambda s: s["write_ms"])
    out["fim_same_ids"] = {"write_ms": spread([s["write_ms"] for s in runs]), "total_ms": spread([s["total_ms"] for s in runs]), "n_out": st["n_out"],
                           "write_ns_per_out_id": round(1e6 * st["write_ms"] / st["n_out"], 6)}
    out["chat_write_vs_fim_write_per_out_id"] = round(out["chat"]["write_ns_per_out_id"] / out["fim_same_ids"]["write_ns_per_out_id"], 3)
    gen.fim_free()
    gen.chat_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
