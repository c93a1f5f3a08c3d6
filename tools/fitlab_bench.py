#!/usr/bin/env python3
"""Dev tool: yabpe_layout_fit_labels on the conversations of tools/chat_bench.py (synth.text_lexicon text generated on the
device, a model trained on the device from it, turns of about --turn-ids ids, --turns of them a conversation, written by
yabpe_chat with drop_oldest to --seq-len), packed whole into rows of --seq-len.  Best of --reps after a warm-up, timed with HIP
events, all in one run:
  * yabpe_layout_fit_labels in the --labels form on yabpe_chat's device results: lengths_ms, write_ms, total_ms, next to a
    device-to-device hipMemcpyAsync of the bytes it must read plus write (ids and labels in, four channels out; the records
    are not in this figure),
  * yabpe_layout_fit on the same sequences' ids, and the two write passes' picoseconds per output byte against each other
    (the labelled call's write_ms holds its place records too),
  * rows and fill against one conversation a row (yabpe_layout_pad to --seq-len),
  * the counters of the call.
   python tools/fitlab_bench.py [--labels shifted|aligned] [--mib 256] [--merges 8000] [--reps 5] [--turn-ids 125] [--turns 8]
                                [--seq-len 2048] [--json out.json]"""
import argparse, ctypes, json, sys
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth

ap = argparse.ArgumentParser()
ap.add_argument("--labels", choices=("shifted", "aligned"), default="shifted")
ap.add_argument("--mib", type=int, default=256)
ap.add_argument("--merges", type=int, default=8000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--turn-ids", type=int, default=125)
ap.add_argument("--turns", type=int, default=8)
ap.add_argument("--seq-len", type=int, default=2048)
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
    roles = np.where(np.arange(n_turns) % a.turns == 0, 0, 1 + (np.arange(n_turns) % a.turns + 1) % 2).astype(np.uint8)  # system, user, assistant, ...
    V, C = len(vocab), a.seq_len
    tpl = dict(heads=[[V, V + 1 + r, V + 4, V + 5] for r in range(3)], feet=[[V + 6, V + 5]] * 3, prefix=[V + 7], train_mask=4, pin_mask=1)
    fi, fl, fo, _fn, n_out, n_convs = gen.chat(di, ni, dd, n_turns, conv_starts, None, roles, **tpl, max_len=C, drop_oldest=True, pin_first=True)
    out = {"text_bytes": tn, "merges": len(merges), "turns": n_turns, "convs": n_convs, "seq_len": C, "labels": a.labels, "chat_ids": n_out,
           "mean_ids_per_conv": round(n_out / n_convs, 1)}
    COUNTERS = ("n_docs", "n_rows", "n_truncated_docs", "n_ids_dropped", "n_pad_slots")
    TIMES = ("lengths_ms", "write_ms", "total_ms")

    def runs_of(call) -> list:
        runs = []
        for k in range(a.reps + 1):
            call()
            if k:
                runs.append(gen.layout_stats())
        return runs

    # ---- the labelled pack on yabpe_chat's device results
    runs = runs_of(lambda: gen.layout_fit_labels(fi, fl, n_out, fo, n_convs, row_len=C, pad_id=V + 8, shifted=a.labels == "shifted", mask_first=True))
    st = min(runs, key=lambda s: s["write_ms"])
    n_slots = st["n_rows"] * C
    moved = 8 * n_out + 16 * n_slots  # ids and labels in, four u32 channels out
    cp = copy_ms(moved // 2, a.reps)  # (a copy of B bytes moves 2 B)
    out["fit_labels"] = {**{t: spread([s[t] for s in runs]) for t in TIMES}, "bytes_read_plus_written": moved, "copy_same_bytes_ms": spread(cp),
                         "write_ms_vs_copy_ms": round(st["write_ms"] / min(cp), 3),
                         "total_ms_vs_copy_ms": round(min(s["total_ms"] for s in runs) / min(cp), 3),
                         "write_ps_per_out_byte": round(1e9 * st["write_ms"] / (16 * n_slots), 4), "counters": {c: st[c] for c in COUNTERS}}
    rows_packed = st["n_rows"]
    # ---- yabpe_layout_fit on the same sequences' ids (three channels out)
    runs = runs_of(lambda: gen.layout_fit(fi, n_out, fo, n_convs, row_len=C, pad_id=V + 8))
    st = min(runs, key=lambda s: s["write_ms"])
    assert st["n_rows"] == rows_packed
    out["fit_ids_only"] = {**{t: spread([s[t] for s in runs]) for t in TIMES}, "write_ps_per_out_byte": round(1e9 * st["write_ms"] / (12 * n_slots), 4)}
    out["fit_labels_write_vs_fit_write_per_out_byte"] = round(out["fit_labels"]["write_ps_per_out_byte"] / out["fit_ids_only"]["write_ps_per_out_byte"], 3)
    # ---- fill: packed rows against one conversation a row
    gen.layout_pad(fi, n_out, fo, n_convs, row_len=C, pad_id=V + 8)
    st = gen.layout_stats()
    out["fill"] = {"packed_rows": rows_packed, "packed_fill": round(n_out / (rows_packed * C), 4), "one_per_row_rows": st["n_rows"],
                   "one_per_row_fill": round(1 - st["n_pad_slots"] / (st["n_rows"] * C), 4)}
    gen.layout_free()
    gen.chat_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
