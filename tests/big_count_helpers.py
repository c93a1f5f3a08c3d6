"""Corpora whose pair counts pass 2^32 through word FREQUENCIES on a few hundred word types (never through large inputs),
and a full-recount reference on Python integers: the high-precision reference of the C oracle at these weights.

The weighted layout keeps one u32 frequency per word (at most 2^32-1, refused above); everything summed from it is 64-bit.
Used by tests/test_big_counts_model.py (CPU), tests/test_gpu_big_counts.py and the `huge_weights` scenario of
tests/dist_workers.py."""
from __future__ import annotations

import random
from collections import Counter
from functools import lru_cache

import numpy as np

from tests import helpers

F_MAX = (1 << 32) - 1  # the largest word frequency the weighted layout takes
SMALL_SEEDS = (1, 2, 3)
LONG_WORDS = [b"a" * 200, b"a" * 201, b"ab" * 100, b"a" * 64, b"ab" * 32 + b"a", b"abc" * 100, b" " * 1500, b"ab" * 700, b"xyxyx" * 13 + b"aaa" * 40]
LONG_FREQS = [F_MAX, F_MAX - 1, F_MAX, 1 << 31, F_MAX, 7, F_MAX, (1 << 31) + 1, F_MAX]


def corpus(seed: int, n_types: int = 240, alphabet: bytes = b"abcde"):
    """-> (distinct words of 2..12 letters, sorted and then shuffled; one frequency in [1, 2^32-1] per word).
    Type i takes its frequency by i % 6: the limit, just under it, around 2^31, a power of two, and twice log-uniform."""
    rng = random.Random(seed)
    words: set[bytes] = set()
    while len(words) < n_types:
        words.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(2, 12))))
    types = sorted(words)
    rng.shuffle(types)
    freqs = []
    for i in range(n_types):
        k = i % 6
        if k == 0:
            f = F_MAX
        elif k == 1:
            f = F_MAX - rng.randrange(1, 1000)
        elif k == 2:
            f = (1 << 31) + rng.randint(-3, 3)
        elif k == 3:
            f = 1 << rng.randrange(32)
        else:
            f = int(2 ** rng.uniform(0, 32))
        freqs.append(min(max(f, 1), F_MAX))
    return tuple(types), tuple(freqs)


@lru_cache(maxsize=None)
def named(name: str):
    """"small1" / "small2" / "small3" (one tile each), "tiles" (20,000 types, many tiles), "long" (words on both sides of
    the 63 / 64 limit, runs of one letter, words past one 1,024-token chunk) -> (types, frequencies)"""
    if name.startswith("small"):
        return corpus(int(name[5:]))
    if name == "tiles":
        return corpus(9, n_types=20000, alphabet=b"abcdefgh")
    if name == "long":
        types, freqs = corpus(4)
        rest = [(w, f) for w, f in zip(types, freqs) if w not in set(LONG_WORDS)]
        return tuple(LONG_WORDS) + tuple(w for w, _ in rest), tuple(LONG_FREQS) + tuple(f for _, f in rest)
    raise KeyError(name)


def freq_array(freqs) -> np.ndarray:
    return np.array(freqs, dtype=np.uint64)


def py_reference(types, freq, n_merges: int, min_frequency: int = 1, specials=(), on_step=None):
    """The full-recount loop of oracle.merge_loop_recount_py, weighted, on Python integers: every pair of every word is
    counted again before every merge, the best is the maximum by (count, (left bytes, right bytes)).
    -> (vocab {bytes: id}, merges [(bytes, bytes)], the count of every merge).  on_step(pair counts, best pair) sees
    every step's whole table before its merge is applied."""
    toks = helpers.base_tokens(specials)
    vocab = {t: i for i, t in enumerate(toks)}
    words: dict[tuple, int] = {}
    for w, f in zip(types, freq):
        key = tuple(bytes([b]) for b in w)
        words[key] = words.get(key, 0) + int(f)
    merges, counts = [], []
    for _ in range(n_merges):
        pc: Counter = Counter()
        for w, f in words.items():
            for j in range(len(w) - 1):
                pc[(w[j], w[j + 1])] += f
        if not pc:
            break
        best = max(pc.items(), key=lambda kv: (kv[1], kv[0]))[0]
        if pc[best] < min_frequency:
            break
        if on_step is not None:
            on_step(pc, best)
        x, y = best
        z = x + y
        new_words: dict[tuple, int] = {}
        for w, f in words.items():
            if x in w:
                out, j = [], 0
                while j < len(w):
                    if j + 1 < len(w) and w[j] == x and w[j + 1] == y:
                        out.append(z)
                        j += 2
                    else:
                        out.append(w[j])
                        j += 1
                w = tuple(out)
            new_words[w] = new_words.get(w, 0) + f
        words = new_words
        merges.append(best)
        counts.append(pc[best])
        if z not in vocab:
            vocab[z] = len(vocab)
    return vocab, merges, counts


def oracle_run(types, freq, n_merges: int, min_frequency: int = 1, specials=()):
    """The C oracle on the same input -> (vocab, merges, ids with "left" / "right" / "merged" / "count"), read-only."""
    from oracle import oracle

    flat, off = helpers.flatten(list(types))
    vocab, merges, ids = oracle.train_flat(flat, off, len(helpers.base_tokens(specials)) + n_merges, min_frequency, list(specials),
                                           return_ids=True, freq=freq_array(freq))
    for a in ids.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, merges, ids


@lru_cache(maxsize=None)
def expected(name: str, n_merges: int, min_frequency: int = 1):
    """The oracle on a named corpus: computed once, shared, left unchanged."""
    return oracle_run(*named(name), n_merges, min_frequency)


@lru_cache(maxsize=None)
def conditions(name: str, n_steps: int = 150) -> dict:
    """What the first n_steps merges of a corpus reach, from the Python-integer reference:
      big         merges with count >= 2^32
      low32_lies  steps where the maximum by (count mod 2^32, bytes) is another pair than the true maximum
      window      steps with a second pair of count >= 2^32 less than 2^31 under the best
      big_ties    consecutive merges with equal counts >= 2^32"""
    out = {"big": 0, "low32_lies": 0, "window": 0, "big_ties": 0}

    def on_step(pc, best):
        c = pc[best]
        out["big"] += c >= 1 << 32
        out["low32_lies"] += max(pc.items(), key=lambda kv: (kv[1] & F_MAX, kv[0]))[0] != best
        out["window"] += any(p != best and v >= 1 << 32 and c - v < 1 << 31 for p, v in pc.items())

    types, freqs = named(name)
    _vocab, _merges, counts = py_reference(types, freqs, n_steps, on_step=on_step)
    out["big_ties"] = sum(1 for a, b in zip(counts, counts[1:]) if a == b and a >= 1 << 32)
    out["counts"] = tuple(counts)
    return out
