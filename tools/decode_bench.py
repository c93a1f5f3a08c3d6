#!/usr/bin/env python3
"""Dev tool: the device decoder (yabpe_decode) on the ids of 1 GiB of synth.text_lexicon text generated on the device, encoded
with a 32,000-merge model trained on the device from that text (yabpe_encode's device results go straight in).  Device time
per phase from yabpe_decode_stats, best of --reps after a warm-up; GB/s of text out; the algorithmic bytes (ids read twice,
text written once) over the device time against the 8 TB/s spec HBM peak and against a device-to-device copy that moves the
same bytes (half read, half written), timed in the same run (torch copy_ between two HBM buffers, HIP events).  A second line decodes the same ids with 1 %
of them replaced by single bytes 0x80-0xFF (the repair path).  For comparison, the plain-Python BBPETokenizer.decode on one
core over a sample of the ids.
   python tools/decode_bench.py [--mib 1024] [--merges 32000] [--reps 3] [--py-ids 4000000] [--json out.json]"""
import argparse, json, subprocess, sys, time
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
sys.path.insert(0, str(REPO))
import numpy as np
from yet_another_bpe import _native, synth
from yet_another_bpe.tokenizer import BBPETokenizer

HBM_PEAK = 8.0e12  # bytes/s, MI355X spec

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--merges", type=int, default=32000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--py-ids", type=int, default=4_000_000)
ap.add_argument("--json", default="")
a = ap.parse_args()


def copy_ms(nbytes: int, reps: int) -> float:
    """Best device time of one device-to-device copy of nbytes (torch copy_ between two HBM buffers, HIP events), in a
    child process of its own so that torch's HIP runtime does not share this one."""
    code = ("import sys, torch\n"
            "n, reps = int(sys.argv[1]), int(sys.argv[2])\n"
            "x = torch.empty(n, dtype=torch.uint8, device='cuda'); y = torch.empty_like(x); y.copy_(x); best = 1e30\n"
            "for _ in range(reps):\n"
            "    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)\n"
            "    e0.record(); y.copy_(x); e1.record(); torch.cuda.synchronize(); best = min(best, e0.elapsed_time(e1))\n"
            "print(best)\n")
    r = subprocess.run([sys.executable, "-c", code, str(nbytes), str(reps)], capture_output=True, text=True, timeout=600, check=True)
    return float(r.stdout.strip().splitlines()[-1])


def timed(ctx, reps, *args, **kw):
    ctx.decode(*args, **kw)  # warm-up
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.decode(*args, **kw)
        wall = time.perf_counter() - t0
        st = ctx.decode_stats()
        st["wall_ms"] = 1e3 * wall
        runs.append(st)
    return min(runs, key=lambda r: r["total_ms"]), runs


def line(best, runs, n_ids, cp_ms):
    phases = ("lengths_ms", "gather_ms", "check_ms", "repair_ms")
    algo = 2 * 4 * n_ids + best["n_bytes"]
    return {"ids": n_ids, "text_bytes_out": best["n_bytes"], "unknown_ids": best["n_unknown"], "replacements": best["n_replacements"],
            "docs_repaired": best["n_docs_repaired"], **{k: round(best[k], 3) for k in phases},
            "device_total_ms": round(best["total_ms"], 3), "call_wall_ms": round(best["wall_ms"], 3),
            "GB_per_s_text": round(best["n_bytes"] / best["total_ms"] / 1e6, 2), "algo_bytes": algo,
            "algo_GB_per_s": round(algo / best["total_ms"] / 1e6, 1), "frac_spec_peak": round(algo / (best["total_ms"] * 1e-3) / HBM_PEAK, 3),
            "copy_same_bytes_ms": round(cp_ms, 3), "copy_GB_per_s": round(algo / cp_ms / 1e6, 1),
            "vs_copy": round(cp_ms / best["total_ms"], 3), "all_total_ms": [round(r["total_ms"], 3) for r in runs]}


lb, lo = synth.text_lexicon(30000, 11)
with _native.Context() as gen:
    tb, _to, _np, tn = gen.synth_generate_lex(a.mib << 20, 11, lb, lo)
    dt, do, nw = gen.pretokenize(tb, n_bytes=tn)
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
    gen.decode_set_model(vocab)
    di, dd, ni = gen.encode(tb, n_bytes=tn)
    best, runs = timed(gen, a.reps, di, n_ids=ni, doc_starts=dd, n_docs=1)
    assert best["n_bytes"] == tn and best["n_replacements"] == 0
    cp = copy_ms((2 * 4 * ni + tn) // 2, a.reps)  # a copy that moves the decoder's algorithmic bytes (half read, half written)
    valid = line(best, runs, ni, cp)
    ids = gen.d2h(di, 4 * ni, np.uint32)
    gen.decode_free()
    rng = np.random.default_rng(7)
    bad = ids.copy()
    m = rng.random(ni) < 0.01
    bad[m] = rng.integers(0x80, 0x100, int(m.sum()), dtype=np.uint32)
    best, runs = timed(gen, a.reps, bad)
    invalid = line(best, runs, ni, cp)
    invalid["replaced_ids"] = int(m.sum())
tok = BBPETokenizer(vocab=vocab, merges=merges)
sample = ids[:a.py_ids].tolist()
t0 = time.perf_counter()
py_text = tok.decode(sample)
py_s = time.perf_counter() - t0
out = {"text_bytes": tn, "merges": len(merges), "valid": valid, "one_percent_invalid": invalid,
       "python_one_core": {"ids": len(sample), "seconds": round(py_s, 3), "ids_per_s": round(len(sample) / py_s),
                           "MB_per_s": round(len(py_text.encode("utf-8")) / py_s / 1e6, 2)}}
print(json.dumps(out))
if a.json:
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1))
