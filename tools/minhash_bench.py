#!/usr/bin/env python3
"""Dev tool: near-duplicate detection (yabpe_minhash) on synth.text_lexicon text generated on the device, encoded with a model
trained on the device from that text; documents cut at pre-token boundaries to a mean of about --doc-ids ids.  The ids never
leave the device.  Best of --reps after a warm-up, all in one run:
  * yabpe_encode's total_ms, then yabpe_minhash's plan_ms / sig_ms / keys_ms / total_ms (HIP events) per --perm value;
  * shingle x function steps per second of the signature kernel (steps = n_shingles * num_perm);
  * the kernel's VALU bound: --wave-cycles issue cycles per inner-loop iteration of a wave (one quad of hashes x two functions
    a lane = 512 steps; the default is the 31 VALU instructions of the disassembly at 4 cycles each) on
    --cus x 4 SIMDs at --mhz, and the share of it reached;
  * the plain-numpy contract (BBPETokenizer.minhash_tokens) on one host core over the first --host-docs documents, checked
    against the device result slot for slot, and the ratio of the two step rates.
   python tools/minhash_bench.py [--mib 256] [--merges 8000] [--reps 3] [--doc-ids 1000] [--perm 128,256] [--json out.json]"""
import argparse, json, sys, time
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
ap.add_argument("--perm", default="128,256")
ap.add_argument("--ngram", type=int, default=5)
ap.add_argument("--host-docs", type=int, default=200)
ap.add_argument("--wave-cycles", type=float, default=124.0, help="issue cycles of one inner-loop iteration of a wave (0: no bound reported)")
ap.add_argument("--cus", type=int, default=256)
ap.add_argument("--mhz", type=float, default=2400.0)
ap.add_argument("--json", default="")
a = ap.parse_args()

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
    step = max(1, round(a.doc_ids * nw / n_all))  # pre-tokens per document
    starts = np.ascontiguousarray(pre_off[:-1:step])
    n_docs = len(starts)
    enc = []
    for k in range(a.reps + 1):  # (the first one is the warm-up)
        di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=starts)
        if k:
            enc.append(gen.encode_stats()["total_ms"])
    out = {"text_bytes": tn, "merges": len(merges), "ids": ni, "docs": n_docs, "mean_ids_per_doc": round(ni / n_docs, 1), "ngram": a.ngram,
           "encode_total_ms": round(min(enc), 3), "runs": []}
    # the host sample: the first documents, copied out once
    hd = min(a.host_docs, n_docs)
    off = gen.d2h(dd, 8 * (hd + 1), np.uint64).astype(np.int64)
    host_ids = gen.d2h(di, 4 * int(off[hd]), np.uint32)
    host_docs = [host_ids[off[d]:off[d + 1]] for d in range(hd)]
    for K in (int(x) for x in a.perm.split(",")):
        bands = K // 4
        runs = []
        for k in range(a.reps + 1):
            ds, _dn, _dk, _nd = gen.minhash(di, ni, dd, n_docs, num_perm=K, ngram=a.ngram, bands=bands, seed=1)
            if k:
                runs.append(gen.minhash_stats())
        st = min(runs, key=lambda s: s["sig_ms"])
        steps = st["n_shingles"] * K
        t0 = time.perf_counter()
        exp_sig, cnt, _keys = BBPETokenizer().minhash_tokens(host_docs, num_perm=K, ngram=a.ngram, seed=1)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(gen.d2h(ds, 4 * hd * K, np.uint32).reshape(hd, K), np.asarray(exp_sig, np.uint32).reshape(hd, K)))
        host_steps = sum(cnt) * K
        run = {"num_perm": K, "bands": bands, "pieces": st["n_pieces"], "shingles": st["n_shingles"], "multi_piece_docs": st["n_multi_piece_docs"],
               "plan_ms": round(st["plan_ms"], 4), "sig_ms": round(st["sig_ms"], 4), "keys_ms": round(st["keys_ms"], 4),
               "total_ms": round(st["total_ms"], 4), "all_sig_ms": [round(s["sig_ms"], 4) for s in runs], "steps": steps,
               "Gsteps_per_s": round(steps / st["sig_ms"] / 1e6, 2), "sig_ms_per_G_shingles": round(st["sig_ms"] / st["n_shingles"] * 1e9, 2),
               "host_numpy": {"docs": hd, "steps": host_steps, "seconds": round(host_s, 3), "Gsteps_per_s": round(host_steps / host_s / 1e9, 4),
                              "equals_device": same}}
        run["device_vs_host_core"] = round(run["Gsteps_per_s"] / max(run["host_numpy"]["Gsteps_per_s"], 1e-9), 1)
        if a.wave_cycles:
            bound_ms = steps / 512 * a.wave_cycles / (a.cus * 4 * a.mhz * 1e6) * 1e3
            run["valu_bound"] = {"wave_cycles_per_512_steps": a.wave_cycles, "cus": a.cus, "mhz": a.mhz, "bound_ms": round(bound_ms, 4),
                                 "share_reached": round(bound_ms / st["sig_ms"], 3)}
        out["runs"].append(run)
    gen.minhash_free()
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
