#!/usr/bin/env python3
"""Dev tool (needs libyabpe_launchprof.so: make -C yet-another-bpe_amd/csrc libyabpe_launchprof.so): what the sparse launches
lose to their slowest workgroup.  Per launch, over the SCAN workgroups: first start, mean end, last end, the same for the end
of the candidate phase, and the candidate tiles per workgroup (mean, max).  last end - mean end, summed over the job, is what
ANY rebalancing between workgroups could save at most.  Options as k=v (yabpe_set_option), e.g. chunk_steal=0.

    python tools/straggler_profile.py [k=v ...]
"""
import ctypes, os, sys
from pathlib import Path
REPO = Path(__file__).resolve().parent.parent
os.environ["YABPE_LIB"] = str(REPO / "yet-another-bpe_amd/csrc/libyabpe_launchprof.so")
sys.path.insert(0, str(REPO / "yet-another-bpe_amd"))
import numpy as np
from yet_another_bpe import _native, synth
spec = synth.SynthSpec.config3(1024 << 20)
base = [bytes([b]) for b in range(256)] + [b"<|endoftext|>"]
opts = [kv.split("=") for kv in sys.argv[1:]]
with _native.Context() as g:
    pb, po, nw, nb = g.synth_generate(spec.target_bytes, spec.n_types, spec.seed, spec.alphabet, spec.space_prefix)
    with _native.Context() as ctx:
        for k, v in opts:
            ctx.set_option(k, int(v))
        ctx.set_vocab(base); ctx.load_words_ptr(pb, po, nw)
        L = _native.lib()
        L.yabpe_debug_launch_profile(None, 1)
        ctx.train(32000, 1)
        st = ctx.stats()
        out = np.zeros(65536 * 4, dtype=np.uint64)
        L.yabpe_debug_launch_profile(ctypes.c_void_p(out.ctypes.data), 0)
        wg = np.zeros(65536 * 8, dtype=np.uint64)
        L.yabpe_debug_launch_wg(ctypes.c_void_p(wg.ctypes.data))
raw = out.reshape(65536, 4)
w = wg.reshape(65536, 8)
print(f"options {dict(opts)}: train {st['train_ms']:.1f} ms, sparse {st['sparse_ms']:.1f} ms, sparse launches {st['sparse_launches']}, second-round pieces taken {st['scan_skip_pieces_taken']}")
valid = np.nonzero((raw[:, 0] != np.uint64(0xFFFFFFFFFFFFFFFF)) & (w[:, 1] != 0))[0]  # row = DevState::iter when the launch started
start = raw[valid, 0].astype(np.float64)
cnt = w[valid, 1].astype(np.float64)
us = lambda x: x / 100.0
span = us(w[valid, 2].astype(np.float64) - start)            # first start -> last scan workgroup's end
mean_end = us(w[valid, 0].astype(np.float64) / cnt - start)  # first start -> the mean scan workgroup's end
cand_last = us(w[valid, 6].astype(np.float64) - start)
cand_mean = us(w[valid, 5].astype(np.float64) / cnt - start)
c_mean = w[valid, 3].astype(np.float64) / cnt
c_max = w[valid, 4].astype(np.float64)
ok = (span > 0) & (span < 50000) & (mean_end > 0)
print("| merges | launches | workgroups | sum span ms | sum (last end - mean end) ms | ... of the candidate phase ms | median span us | median last - mean us | candidates per workgroup mean | mean of the launches' max |")
print("|---|---|---|---|---|---|---|---|---|---|")
rows = [(46, 100), (100, 300), (300, 1000), (1000, 3000), (3000, 8000), (8000, 12000), (12000, 20000), (20000, 32000), (0, 65536)]
for lo, hi in rows:
    m = ok & (valid >= lo) & (valid < hi)
    if not m.any():
        continue
    name = "whole job" if hi == 65536 else f"{lo}-{hi}"
    print(f"| {name} | {m.sum()} | {np.median(cnt[m]):.0f} | {span[m].sum() / 1000:.1f} | {(span[m] - mean_end[m]).sum() / 1000:.1f} | {(cand_last[m] - cand_mean[m]).sum() / 1000:.1f} | "
          f"{np.median(span[m]):.1f} | {np.median(span[m] - mean_end[m]):.1f} | {c_mean[m].mean():.1f} | {c_max[m].mean():.1f} |")
