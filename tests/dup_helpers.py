"""Hand-built ragged id corpora the exact-substring tests share (test_dupspans_api.py on the CPU, test_gpu_dupspans.py on the
GPU), and the brute-force rule: every window against every earlier one, O(N^2 n), kept apart from the dict of the package."""
from __future__ import annotations

import functools

import numpy as np

MIN_LENS = (1, 2, 5, 50, 64, 1024)
CORPORA = ("seams", "runs", "tiles", "hot")


def _rand(rng, k):
    """k ids, almost surely without a repeated window of any length"""
    return rng.integers(1000, 1 << 32, k, dtype=np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def corpus(name: str, n: int) -> tuple:
    """-> the documents (tuples of ids) of corpus `name` for min_len = n"""
    rng = np.random.default_rng(n * 7 + len(name))
    if name == "seams":  # lengths n - 1, n, n + 1; empty documents first, in the middle and last; ids 0 and 0xFFFFFFFF
        a, b = _rand(rng, n), _rand(rng, n + 3)
        edge = [0, 0xFFFFFFFF] * n
        docs = [[], _rand(rng, n - 1), a, _rand(rng, n + 1), [], a,  # (a again: a repeat across two documents)
                b + _rand(rng, 2) + b + _rand(rng, 1) + a[:n - 1],   # a repeat inside one document; n - 1 of a: none
                a[1:] + b[:1], edge, []]
    elif name == "runs":  # the overlap predicate; a periodic document whose period does not divide n
        period = next(k for k in (2, 3) if n % k)
        docs = [[7] * (n + 1), [8] * (2 * n - 1), [9] * (2 * n), [5] * (2 * n + 1), (list(range(20, 20 + period)) * (2 * n))[:2 * n + period + 1]]
    elif name == "tiles":  # about 3,100 ids: a repeat window starts at the last position of the first 1,024-tile, another one
        src, big = _rand(rng, n + 2), _rand(rng, 3100)  # ends the document, a third lies across the second tile's end
        big[1023:1023 + n] = src[1:1 + n]
        big[2040:2040 + n] = src[2:2 + n] if 2040 + 2 * n <= 3100 else big[2040:2040 + n]
        big[3100 - n:] = src[:n]
        docs = [_rand(rng, 3), src, big]
    else:  # "hot": 200 identical short documents, every window of all but the first on one slot's chain
        docs = [_rand(rng, n + 1)] * 200
    return tuple(tuple(d) for d in docs)


def flat(docs):
    """-> (ids np.uint32[n_ids], doc_off np.uint64[n_docs + 1])"""
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.asarray([t for d in docs for t in d], dtype=np.uint32), off


@functools.lru_cache(maxsize=None)
def brute(name: str, n: int):
    """-> (masks, n_dup, n_windows, n_repeats) of corpus(name, n) by comparing each window with every earlier one."""
    docs = corpus(name, n)
    ids, off = flat(docs)
    win = np.lib.stride_tricks.sliding_window_view(ids, n) if len(ids) >= n else np.zeros((0, n), np.uint32)
    starts = [p for d in range(len(docs)) for p in range(int(off[d]), int(off[d + 1]) - n + 1)]
    starts = np.asarray(starts, dtype=np.int64)
    mask = np.zeros(len(ids), np.uint8)
    n_repeats = 0
    for k, p in enumerate(starts.tolist()):
        earlier = starts[:k][starts[:k] + n <= p]  # the windows that end at or before p
        earlier = earlier[win[earlier, 0] == win[p, 0]]  # (the first id decides most of them; then id by id)
        if len(earlier) and (win[earlier] == win[p]).all(axis=1).any():
            n_repeats += 1
            mask[p:p + n] = 1
    masks = [mask[int(off[d]):int(off[d + 1])].tolist() for d in range(len(docs))]
    return masks, [sum(m) for m in masks], len(starts), n_repeats
