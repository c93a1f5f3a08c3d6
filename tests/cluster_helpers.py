"""Hand-built signature and key arrays the cluster tests share (test_cluster_api.py on the CPU, test_gpu_cluster.py on the GPU).
minhash_clusters takes keys as given, so no documents are needed: rows are random (all keys distinct, no slot agrees) and the
structure is planted on top."""
from __future__ import annotations

import numpy as np

SHAPES = ((1, 1), (64, 16), (100, 100), (128, 32), (1024, 1024))  # (num_perm K, bands B)
CORPORA = ("unique", "identical", "bucket_and_chains", "no_shingles", "cross_band")


def mid(K: int) -> int:
    """The min_agree that rejects some planted edges: planted rows agree with their base in K, mid(K) or mid(K) - 1 slots."""
    return (K + 1) // 2


def corpus(name: str, K: int, B: int, n: int = 300):
    """-> (sig u32[n, K], keys u64[n, B], n_shingles u64[n] or None)"""
    rng = np.random.default_rng(K * 1031 + B)
    sig = rng.integers(0, 1 << 32, (n, K), dtype=np.uint32)
    keys = rng.integers(0, 1 << 63, (n, B), dtype=np.uint64)
    cnt = None
    if name == "identical":  # every atomicMin on B addresses; everything hooks under 0
        sig[:], keys[:] = sig[0], keys[0]
    elif name != "unique":  # planted rows: the base row in the first K, mid or mid - 1 slots
        for d in range(10, n):
            sig[d, :(K, mid(K), mid(K) - 1)[d % 3]] = sig[0, :(K, mid(K), mid(K) - 1)[d % 3]]
    if name == "bucket_and_chains":
        keys[10:100, 0] = keys[10, 0]  # one bucket of 90 members
        for i in range(1, 41):  # d ~ d - 1 in band i % B: a chain across the bands, labelled by its first document
            keys[200 + i, i % B] = keys[199 + i, i % B]
        keys[260:270, :] = keys[260, :]  # the same pair from every band: one candidate
        for t in range(B):  # up to 150 distinct anchors for one document, repeated across rounds of 64 bands; 7, repeated inside a round
            keys[290, t], keys[291, t] = keys[t % 150, t], keys[t % 7, t]
    elif name == "no_shingles":  # identical rows, every third one of a document without shingles; the first one among them
        keys[50:150] = keys[50]
        cnt = np.ones(n, np.uint64)
        cnt[50:150:3] = 0
        cnt[[0, n - 1]] = 0
    elif name == "cross_band":
        keys[20, 0] = keys[21, (B - 1)] = 12345  # an equal value in two bands: no bucket (B > 1)
        keys[100:200, :] = 777  # one value in every band: B buckets, and residents of another band with the probing entry's key
        keys[30:35, B - 1] = keys[40, 0]  # the last band; its value also stands in band 0 of another document
    return sig, keys, cnt
