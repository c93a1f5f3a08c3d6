#!/usr/bin/env python3
"""Dev tool: the fixed-shape batch layouts (yabpe_layout_pad / yabpe_layout_pack / yabpe_layout_windows) on the ids of 1 GiB of
synth.text_lexicon text generated on the device, encoded with a 32,000-merge model trained on the device from that text;
documents cut at pre-token boundaries to a mean of about 1,000 ids.  Encode once, then every layout, best of --reps after a
warm-up: device time per phase from yabpe_layout_stats, bytes read + written over write_ms as GB/s, and that rate against a plain
device-to-device hipMemcpyAsync of the same number of output bytes (HIP events, same run).  Padded: max_length 1024; packed:
seq_len 2048 with an EOS; windows: max_length 1024, stride 128, a BOS, without spans and with the byte spans of
yabpe_encode_spans.  For comparison, what a user does without the layout calls on a --host-mib sample: encode_array, then a
numpy loop per document on the host that builds the same padded batch.
--pairs: only yabpe_layout_pairs, on the same ids with the documents paired two by two, <s> A </s></s> B </s>: longest_first at
the max_length that cuts about half the pairs, and windows at max_length 1536 with stride 128 (about three rows a pair: the
first side of about 1,000 ids is in every row), each without and with byte spans;
the device time of the phases and the output bytes per second of the write pass (4 B of ids + 1 B of type a slot, + 16 B with
spans), next to the same figure of yabpe_layout_windows at the same row length and stride on the same ids.
--fit: only yabpe_layout_fit (whole documents, best-fit decreasing) next to yabpe_layout_pack on the same ids, both at seq_len 2048
with an EOS: rows and pad slots of both, the device time of the phases, the bytes read + written over write_ms of both write
passes and their ratio; the plan of the same histogram run once more on the host through the CPU model of the rules
(tests/hostmodel/fit_model.cpp, the same fit_plan the driver calls) for its shapes, steps and wall time.
   python tools/layout_bench.py [--mib 1024] [--merges 32000] [--reps 3] [--host-mib 64] [--pairs | --fit] [--json out.json]"""
import argparse, ctypes, json, subprocess, sys, time
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth
from yet_another_bpe.tokenizer import BBPETokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--merges", type=int, default=32000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host-mib", type=int, default=64)
ap.add_argument("--doc-ids", type=int, default=1000)
ap.add_argument("--pairs", action="store_true")
ap.add_argument("--fit", action="store_true")
ap.add_argument("--json", default="")
a = ap.parse_args()
PAD_LEN, PACK_LEN, EOS = 1024, 2048, 2
WIN_LEN, WIN_STRIDE, BOS = 1024, 128, 1
PAIR_WIN_LEN, PAIR_STRIDE, SEP, PAIR_ADDED = 1536, 128, 3, 4  # <s> A </s></s> B </s>


def emit(out: dict) -> None:
    print(json.dumps(out))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))


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
    for _ in range(reps + 1):  # (the first one is the warm-up)
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(n_bytes), 3, None))
        ok(hip.hipEventRecord(e1, None)); ok(hip.hipEventSynchronize(e1)); ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        best = min(best, ms.value) if _ else best
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
    gen.encode(tb, n_bytes=tn, doc_starts=starts)  # warm-up
    di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=starts)
    enc = gen.encode_stats()
    doc_off = gen.d2h(dd, 8 * (n_docs + 1), np.uint64).astype(np.int64)

    def timed(call):
        call()  # warm-up
        runs = []
        for _ in range(a.reps):
            call()
            runs.append(gen.layout_stats())
        return min(runs, key=lambda r: r["total_ms"]), [round(r["total_ms"], 3) for r in runs]

    def report(st, all_ms, read_b, write_b):
        cp = copy_ms(write_b, a.reps)
        rate, cp_rate = (read_b + write_b) / st["write_ms"] / 1e6, 2 * write_b / cp / 1e6
        return {"rows": st["n_rows"], "row_len": st["row_len"], "truncated_docs": st["n_truncated_docs"], "ids_dropped": st["n_ids_dropped"],
                "pad_slots": st["n_pad_slots"], "lengths_ms": round(st["lengths_ms"], 3), "write_ms": round(st["write_ms"], 3),
                "total_ms": round(st["total_ms"], 3), "all_total_ms": all_ms, "bytes_read": read_b, "bytes_written": write_b,
                "write_GB_per_s": round(rate, 1), "copy_same_output_bytes_ms": round(cp, 3), "copy_GB_per_s": round(cp_rate, 1),
                "write_rate_vs_copy": round(rate / cp_rate, 3), "write_ms_vs_copy_ms": round(st["write_ms"] / cp, 2),
                "total_vs_encode_emit_ms": round(st["total_ms"] / enc["emit_ms"], 3),
                "write_ns_per_slot": round(st["write_ms"] * 1e6 / max(1, st["n_rows"] * st["row_len"]), 5)}

    lens = np.diff(doc_off)
    if a.pairs:
        n_even = n_docs - n_docs % 2  # (an odd last document joins the one before it: the last document ends at n_ids)
        sums = lens[:n_even].copy()
        sums[-1] = ni - doc_off[n_even - 1]
        la, lb = sums[0::2], sums[1::2]
        sums = la + lb
        Cb = PAIR_WIN_LEN - PAIR_ADDED - np.minimum(la, PAIR_WIN_LEN - PAIR_ADDED - PAIR_STRIDE - 1)
        n_pair_win = int(np.where(lb <= Cb, 1, 1 + -(-(lb - Cb) // (Cb - PAIR_STRIDE))).sum())
        assert n_pair_win * PAIR_WIN_LEN < 1 << 32, f"{n_pair_win} window rows: first sides too long for max_length {PAIR_WIN_LEN}"
        cut_len = int(np.median(sums)) + PAIR_ADDED
        di, dd, ds, ni_s = gen.encode_spans(tb, n_bytes=tn, doc_starts=starts)
        assert ni_s == ni

        def phases(st, all_ms, slot_bytes):
            out_b = slot_bytes * st["n_rows"] * st["row_len"]
            return {"rows": st["n_rows"], "row_len": st["row_len"], "truncated": st["n_truncated_docs"], "ids_dropped": st["n_ids_dropped"],
                    "pad_slots": st["n_pad_slots"], "lengths_ms": round(st["lengths_ms"], 3), "write_ms": round(st["write_ms"], 3),
                    "total_ms": round(st["total_ms"], 3), "all_total_ms": all_ms, "write_pass_output_bytes": out_b,
                    "write_pass_output_GB_per_s": round(out_b / st["write_ms"] / 1e6, 1)}

        out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "pairs": n_even // 2, "median_ids_per_pair": int(np.median(sums))}
        for name, L, mode, stride in ((f"longest_first_{cut_len}", cut_len, "longest_first", 0),
                                      (f"windows_{PAIR_WIN_LEN}_stride_{PAIR_STRIDE}", PAIR_WIN_LEN, "windows", PAIR_STRIDE)):
            kw = dict(row_len=L, mode=mode, stride=stride, sep_id=SEP, n_sep=2, pad_id=0, bos_id=BOS, eos_id=EOS)
            for spans, tag in ((None, ""), (ds, "_byte_spans")):
                st, all_ms = timed(lambda: gen.layout_pairs(di, ni, dd, n_even, spans, **kw))
                assert mode != "windows" or st["n_rows"] == n_pair_win
                pairs = phases(st, all_ms, 21 if spans else 5)
                st, all_ms = timed(lambda: gen.layout_windows(di, ni, dd, n_docs, spans, row_len=L, stride=stride, pad_id=0, bos_id=BOS))
                yard = phases(st, all_ms, 20 if spans else 4)
                pairs["write_rate_vs_layout_windows"] = round(pairs["write_pass_output_GB_per_s"] / yard["write_pass_output_GB_per_s"], 3)
                out["pairs_" + name + tag] = pairs
                out["layout_windows_" + str(L) + "_stride_" + str(stride) + tag] = yard
        gen.layout_free()
        emit(out)
        sys.exit(0)
    if a.fit:
        hm = REPO / "tests" / "hostmodel"
        if not (hm / "libfit_model.so").exists():
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(hm / "libfit_model.so"), str(hm / "fit_model.cpp")])
        model = ctypes.CDLL(str(hm / "libfit_model.so"))
        kept = np.minimum(lens + 1, PACK_LEN)  # n_d: the EOS survives the cut
        hist = np.bincount(kept, minlength=PACK_LEN + 1).astype(np.uint32)
        first, place, pl = np.zeros(n_docs + 2, np.uint64), np.zeros(n_docs + 2, np.uint32), np.zeros(4 * (n_docs + 2), np.uint32)
        ns, npl, nr, steps = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        plan_ms = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = model.fit_model_plan(ctypes.c_void_p(hist.ctypes.data), ctypes.c_uint32(PACK_LEN), ctypes.c_void_p(first.ctypes.data),
                                      ctypes.c_void_p(place.ctypes.data), ctypes.c_void_p(pl.ctypes.data), ctypes.c_uint32(n_docs + 2),
                                      ctypes.c_uint32(n_docs + 2), ctypes.byref(ns), ctypes.byref(npl), ctypes.byref(nr), ctypes.byref(steps))
            plan_ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        kw = dict(row_len=PACK_LEN, pad_id=0, eos_id=EOS)
        out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "docs": n_docs, "mean_ids_per_doc": round(ni / n_docs, 1), "seq_len": PACK_LEN,
               "plan": {"shapes": ns.value, "places": npl.value, "steps": steps.value, "rows": nr.value,
                        "host_wall_ms_best": round(min(plan_ms[1:]), 3), "host_wall_ms_all": [round(t, 3) for t in plan_ms[1:]]}}
        # bytes a write pass moves: the ids it keeps, the document starts (and the sorted documents), 12 B a slot (and `used`)
        reads = {"pack": 4 * ni + 8 * (n_docs + 1), "fit": 4 * int((kept - 1).sum()) + 8 * (n_docs + 1) + 4 * n_docs}
        for name, call in (("pack", gen.layout_pack), ("fit", gen.layout_fit)):
            st, all_ms = timed(lambda: call(di, ni, dd, n_docs, **kw))
            n_slots = st["n_rows"] * PACK_LEN
            moved = reads[name] + 12 * n_slots + (4 * st["n_rows"] if name == "fit" else 0)
            out[name] = {"rows": st["n_rows"], "pad_slots": st["n_pad_slots"], "fill": round(1 - st["n_pad_slots"] / max(1, n_slots), 5),
                         "truncated_docs": st["n_truncated_docs"], "ids_dropped": st["n_ids_dropped"], "lengths_ms": round(st["lengths_ms"], 3),
                         "write_ms": round(st["write_ms"], 3), "total_ms": round(st["total_ms"], 3), "all_total_ms": all_ms,
                         "host_gap_ms": round(st["total_ms"] - st["lengths_ms"] - st["write_ms"], 3), "write_bytes": moved,
                         "write_GB_per_s": round(moved / st["write_ms"] / 1e6, 1)}
        assert out["fit"]["rows"] == nr.value
        out["fit_write_rate_vs_pack_write"] = round(out["fit"]["write_GB_per_s"] / out["pack"]["write_GB_per_s"], 3)
        gen.layout_free()
        emit(out)
        sys.exit(0)
    st, all_ms = timed(lambda: gen.layout_pad(di, ni, dd, n_docs, row_len=PAD_LEN, pad_id=0))
    padded = report(st, all_ms, 4 * int(np.minimum(lens, PAD_LEN).sum()) + 8 * n_docs, 4 * n_docs * PAD_LEN + 4 * n_docs)
    st, all_ms = timed(lambda: gen.layout_pack(di, ni, dd, n_docs, row_len=PACK_LEN, pad_id=0, eos_id=EOS))
    packed = report(st, all_ms, 4 * ni + 8 * (n_docs + 1), 12 * st["n_rows"] * PACK_LEN)
    # windows: every kept content id is read once per row that holds it, plus one 16-byte record per row
    C, step = WIN_LEN - 1, WIN_LEN - 1 - WIN_STRIDE
    win_rows = np.where(lens <= C, 1, 1 + -(-(lens - C) // step))
    kept = int((lens + (win_rows - 1) * WIN_STRIDE).sum())
    n_win = int(win_rows.sum())
    win_kw = dict(row_len=WIN_LEN, stride=WIN_STRIDE, pad_id=0, bos_id=BOS)
    st, all_ms = timed(lambda: gen.layout_windows(di, ni, dd, n_docs, **win_kw))
    assert st["n_rows"] == n_win and st["n_pad_slots"] == n_win * WIN_LEN - kept - n_win
    windows = report(st, all_ms, 4 * kept + 16 * n_win, 4 * n_win * WIN_LEN)
    di, dd, ds, ni_s = gen.encode_spans(tb, n_bytes=tn, doc_starts=starts)
    assert ni_s == ni
    st, all_ms = timed(lambda: gen.layout_windows(di, ni, dd, n_docs, ds, **win_kw))
    windows_spans = report(st, all_ms, 20 * kept + 16 * n_win, 20 * n_win * WIN_LEN)
    gen.layout_free()
    n_host = int(np.searchsorted(starts, a.host_mib << 20))  # the documents that lie inside the host sample
    sample = gen.d2h(tb, int(starts[n_host]) if n_host < n_docs else tn).tobytes()
    cuts = starts[:n_host].tolist() + [len(sample)]

docs = [sample[p:q].decode("utf-8") for p, q in zip(cuts, cuts[1:])]
tok = BBPETokenizer(vocab=vocab, merges=merges)
tok.encode_array_padded(docs[:8], PAD_LEN, pad_id=0)  # (model upload, warm-up)
t0 = time.perf_counter()
rows_dev, _len = tok.encode_array_padded(docs, PAD_LEN, pad_id=0)
dev_s = time.perf_counter() - t0
t0 = time.perf_counter()
ids, off = tok.encode_array(docs)
enc_s = time.perf_counter() - t0
rows = np.zeros((len(docs), PAD_LEN), dtype=np.uint32)
for d in range(len(docs)):  # what a user writes today: one slice and one assignment per document
    s = ids[off[d]:off[d + 1]][:PAD_LEN]
    rows[d, :len(s)] = s
host_s = time.perf_counter() - t0
assert np.array_equal(rows, rows_dev)
out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "docs": n_docs, "mean_ids_per_doc": round(ni / n_docs, 1),
       "encode_emit_ms": round(enc["emit_ms"], 3), "encode_total_ms": round(enc["total_ms"], 3), "padded_1024": padded,
       "packed_2048_eos": packed, "windows_1024_stride_128_bos": windows, "windows_1024_stride_128_bos_byte_spans": windows_spans,
       "host_sample": {"text_bytes": len(sample), "docs": len(docs), "encode_array_then_numpy_loop_s": round(host_s, 3),
                       "of_which_encode_array_s": round(enc_s, 3), "MB_per_s": round(len(sample) / host_s / 1e6, 1),
                       "encode_array_padded_s": round(dev_s, 3), "encode_array_padded_MB_per_s": round(len(sample) / dev_s / 1e6, 1)}}
emit(out)
