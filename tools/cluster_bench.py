#!/usr/bin/env python3
"""Dev tool: near-duplicate clusters (yabpe_minhash_cluster), HIP events inside the call, best of --reps after a warm-up, all in
one run:
  (a) the corpus of tools/minhash_bench.py (synth.text_lexicon text generated, trained on and encoded on the device, documents
      of about --doc-ids ids), signatures with K = 128 and 32 bands; a --planted share of the rows is then replaced by
      near-copies of earlier rows (10 % of the slots redrawn, keys folded again from the row: the rule of minhash_logic.h in
      numpy) and the call runs with min_agree 0 and --agree (about 0.8 K); yabpe_minhash's time of the same run beside it;
  (b) synthetic keys without duplicates for the --synthetic document counts (32 bands, min_agree 0);
  (c) --identical documents with one and the same row (every atomicMin on 32 addresses), min_agree 0 and --agree.
Per case: preset / insert / link / flatten / total ms, entries per second of the insert, the same-run floor (tools/cluster_floor:
one random 4-byte atomicMin per entry into a table of the same size) and insert_ms over it, and the plain-Python rule
(BBPETokenizer.minhash_clusters) on one host core over the first --host-docs documents, checked against the device's result
for those documents label for label and statistic for statistic.
   python tools/cluster_bench.py [--mib 256] [--reps 5] [--synthetic 1000000,10000000] [--out profiles/cluster_bench.txt]"""
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
ap.add_argument("--planted", type=float, default=0.2)
ap.add_argument("--agree", type=int, default=102)
ap.add_argument("--synthetic", default="1000000,10000000")
ap.add_argument("--identical", type=int, default=1000000)
ap.add_argument("--host-docs", type=int, default=20000)
ap.add_argument("--out", default="")
a = ap.parse_args()
K, B = 128, 32
TOK = BBPETokenizer()
floor_bin = REPO / "tools" / "cluster_floor"
if not floor_bin.exists():
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", str(floor_bin), str(REPO / "tools" / "cluster_floor.hip")])
lines = []


def case(ctx, name, sig, keys, cnt, n, m, extra=None):
    """One measured case: sig / keys / cnt host arrays or device pointers of n documents."""
    runs = []
    for k in range(a.reps + 1):  # (the first one is the warm-up)
        ctx.minhash_cluster(sig, keys, cnt, n, num_perm=K, bands=B, min_agree=m)
        if k:
            runs.append(ctx.minhash_cluster_stats())
    st = min(runs, key=lambda s: s["total_ms"])
    lg = st["n_slots"].bit_length() - 1
    floor = json.loads(subprocess.check_output([str(floor_bin), str(lg), str(max(st["n_entries"], 1)), str(a.reps)], timeout=300))
    out = {"case": name, "min_agree": m, **{k: v for k, v in st.items() if not k.endswith("_ms")},
           **{k: round(st[k], 4) for k in ("preset_ms", "insert_ms", "link_ms", "flatten_ms", "total_ms")},
           "all_insert_ms": [round(s["insert_ms"], 4) for s in runs], "M_entries_per_s_insert": round(st["n_entries"] / max(st["insert_ms"], 1e-9) / 1e3, 1),
           "floor_atomic_min_ms": floor["atomic_min_ms"], "insert_over_floor": round(st["insert_ms"] / max(floor["atomic_min_ms"], 1e-9), 2)}
    if isinstance(keys, np.ndarray):  # the host rule over a sample, against the device on the same sample
        hd = min(a.host_docs, n)
        hs, hk, hc = (None if x is None else x[:hd] for x in (sig if m else None, keys, cnt))
        t0 = time.perf_counter()
        exp, exp_st = TOK.minhash_clusters(hs, hk, hc, min_agree=m)
        host_s = time.perf_counter() - t0
        got = ctx.minhash_cluster_to_host(hs, hk, hc, hd, num_perm=K, bands=B, min_agree=m)
        dst = ctx.minhash_cluster_stats()
        out["host_rule"] = {"docs": hd, "seconds": round(host_s, 3), "device_total_ms": round(dst["total_ms"], 4),
                            "equals_device": bool(got.tolist() == exp and all(dst[k] == v for k, v in exp_st.items()))}
    out.update(extra or {})
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)


# (a) text -> ids -> signatures on the device, as tools/minhash_bench.py
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
    starts = np.ascontiguousarray(pre_off[:-1:max(1, round(a.doc_ids * nw / n_all))])
    di, dd, ni = gen.encode(tb, n_bytes=tn, doc_starts=starts)
    enc_ms = gen.encode_stats()["total_ms"]
    mh = []
    for k in range(a.reps + 1):
        ds, dn, dk, nd = gen.minhash(di, ni, dd, len(starts), num_perm=K, ngram=5, bands=B, seed=1)
        if k:
            mh.append(gen.minhash_stats()["total_ms"])
    same_run = {"text_bytes": tn, "ids": ni, "encode_total_ms": round(enc_ms, 3), "minhash_total_ms": round(min(mh), 4)}
    case(gen, "corpus, device pointers of yabpe_minhash", ds, dk, dn, nd, 0, same_run)
    case(gen, "corpus, device pointers of yabpe_minhash", ds, dk, dn, nd, a.agree, same_run)
    sig = gen.d2h(ds, 4 * nd * K, np.uint32).reshape(nd, K)
    cnt = gen.d2h(dn, 8 * nd, np.uint64)
    gen.minhash_free()
    rng = np.random.default_rng(5)
    copies = rng.choice(np.arange(1, nd), int(a.planted * nd), replace=False)
    sig[copies] = sig[(rng.random(len(copies)) * copies).astype(np.int64)]  # an earlier row ...
    redraw = rng.random((len(copies), K)) < 0.1                             # ... with a tenth of its slots redrawn
    sig[copies] = np.where(redraw, rng.integers(0, 1 << 32, redraw.shape, dtype=np.uint32), sig[copies])
    keys = np.empty((nd, B), np.uint64)
    for t in range(B):
        s = np.full(nd, synth.rnd_int(0, 0x6B, t), np.uint64)
        for j in range(K // B):
            s = synth.rnd(s, 0, sig[:, t * (K // B) + j].astype(np.uint64))
        keys[:, t] = s
    for m in (0, a.agree):
        case(gen, f"corpus, {a.planted:.0%} of the rows planted near-copies", sig, keys, cnt, nd, m, same_run)
    # (b) synthetic keys without duplicates
    for n in (int(x) for x in a.synthetic.split(",") if x):
        keys = rng.integers(0, 1 << 63, (n, B), dtype=np.uint64)
        case(gen, f"synthetic, {n} documents without duplicates", None, keys, None, n, 0)
    # (c) one row for everybody
    n = a.identical
    keys = np.tile(rng.integers(0, 1 << 63, (1, B), dtype=np.uint64), (n, 1))
    sig = np.tile(rng.integers(0, 1 << 32, (1, K), dtype=np.uint32), (n, 1))
    for m in (0, a.agree):
        case(gen, f"identical, {n} documents with one row", sig, keys, None, n, m)
    gen.minhash_cluster_free()
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
