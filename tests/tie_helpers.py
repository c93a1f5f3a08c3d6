"""Small tie-heavy corpora for the batched selection (select_eval) and a plain-Python sequential BPE replay that says what
each of them reaches.  Everything is deterministic (random.Random with fixed seeds); nothing here touches a GPU.

  stems    word types that share 9-14-byte stems over "abcdef" and differ in a 1-4-byte tail, few distinct frequencies: the
           merged tokens soon share their first eight bytes, so the tie rule's prefix comparison cannot tell ("undecided")
  plateau  short word types of random bytes with two frequencies: more than WIN = 128 distinct pairs tie at the top
  levels   short word types with slowly rising frequencies: the top count level is small, more than 128 pairs lie close under it
  reuse    tiny alphabets with specials like "ab": merged bytes that are a token already (the merge takes that id)

tools/batch_sim.cpp shows on the CPU that `stems` tells the device's tie rule from two subtly wrong ones
(tests/test_batch_rule.py); replay() gives the conditions the GPU tests assert about their inputs."""
from __future__ import annotations

import random
from collections import Counter
from functools import lru_cache

import numpy as np

WIN = 128  # the selection's window (csrc/yabpe_kernels.h)


def _occurrences(types: list[bytes], freqs: list[int], seed: int) -> list[bytes]:
    words = [w for w, f in zip(types, freqs) for _ in range(f)]
    random.Random(seed).shuffle(words)
    return words


@lru_cache(maxsize=None)
def stems_types(seed: int = 10) -> tuple[tuple[bytes, ...], tuple[int, ...]]:
    """-> (word types, their frequencies): 24 stems, 4-8 distinct tails each, frequencies from {40, 40, 40, 80}."""
    rng = random.Random(seed)
    types: list[bytes] = []
    for _ in range(24):
        stem = bytes(rng.choice(b"abcdef") for _ in range(rng.randint(9, 14)))
        tails, n_tails = set(), rng.randint(4, 8)
        while len(tails) < n_tails:
            tails.add(bytes(rng.choice(b"abcdef") for _ in range(rng.randint(1, 4))))
        types += [stem + t for t in sorted(tails)]
    types = list(dict.fromkeys(types))
    rng.shuffle(types)
    return tuple(types), tuple(rng.choice((40, 40, 40, 80)) for _ in types)


def stems(seed: int = 10) -> list[bytes]:
    """Every occurrence, shuffled (the flat and device-dedup layouts)."""
    types, freqs = stems_types(seed)
    return _occurrences(list(types), list(freqs), seed + 1)


def stems_pooled(mult: int = 1, seed: int = 10) -> tuple[list[bytes], np.ndarray]:
    """(unique words, freq * mult) for the weighted layout; mult = 1000 lifts cmax >> win_shift above kmax."""
    types, freqs = stems_types(seed)
    return list(types), np.array(freqs, dtype=np.uint64) * np.uint64(mult)


def _short_types(n: int, seed: int) -> list[bytes]:
    rng = random.Random(seed)
    seen: dict[bytes, None] = {}
    while len(seen) < n:
        seen[bytes(rng.sample(range(33, 250), rng.randint(2, 4)))] = None  # (distinct bytes inside a word: no a == b runs)
    return list(seen)


@lru_cache(maxsize=None)
def plateau_types(seed: int = 31) -> tuple[tuple[bytes, ...], tuple[int, ...]]:
    types = _short_types(260, seed)
    rng = random.Random(seed + 1)
    return tuple(types), tuple(rng.choice((48, 96)) for _ in types)


def plateau(seed: int = 31) -> list[bytes]:
    types, freqs = plateau_types(seed)
    return _occurrences(list(types), list(freqs), seed + 2)


@lru_cache(maxsize=None)
def levels_types(seed: int = 41) -> tuple[tuple[bytes, ...], tuple[int, ...]]:
    types = _short_types(400, seed)
    return tuple(types), tuple(1000 + t // 12 for t in range(len(types)))


def levels(seed: int = 41) -> list[bytes]:
    types, freqs = levels_types(seed)
    return _occurrences(list(types), list(freqs), seed + 2)


@lru_cache(maxsize=None)
def reuse_cases() -> tuple[tuple[str, tuple[bytes, ...], tuple[int, ...], tuple[str, ...]], ...]:
    """-> (name, word types, frequencies >= 20, specials).  The specials' bytes come up as merged bytes during training: a few
    frequent words in front make sure of it, random words over the alphabet follow."""
    out = []
    for name, alphabet, specials, first, seed in (
            ("ab_ab", b"ab", ("ab",), (), 51),
            ("ab_a_b", b"ab", ("a", "b"), (), 52),  # (specials that are base tokens already: no id, no reuse)
            ("abc_abc_bc", b"abc", ("abc", "bc"), (b"abcabc", b"bcbc", b"abc"), 53),
            ("abc_many", b"abc", ("ab", "bc", "ca", "abc", "bca", "cab", "abca", "bcab"), (), 54),
            # independent pairs in front of the specials' bytes: a reused id falls behind the first position of a batch
            ("abcdef_pairs", b"abcdef", ("cd", "ef", "abcd", "cdef", "efab"),
             (b"abcdef", b"cdefab", b"efabcd", b"abcd", b"cdef", b"efab", b"ab", b"cd", b"ef"), 55)):
        rng = random.Random(seed)
        seen: dict[bytes, None] = dict.fromkeys(first)
        while len(seen) < 40:
            seen[bytes(rng.choice(alphabet) for _ in range(rng.randint(2, 12)))] = None
        types = list(seen)
        freqs = [300 - 10 * k if k < len(first) else rng.randint(20, 60) for k in range(len(types))]
        out.append((name, tuple(types), tuple(freqs), specials))
    return tuple(out)


def base_tokens(specials) -> list[bytes]:
    toks = [bytes([b]) for b in range(256)]
    for s in specials:
        tb = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        if tb not in toks:
            toks.append(tb)
    return toks


def replay(types, freqs, specials=(), num_merges: int = 1 << 30, min_frequency: int = 1) -> list[dict]:
    """Sequential BPE on (word types, frequencies), plain Python, a full recount per step.  One dict per merge:
      count   the best count                          at_top  distinct pairs with that count
      near    distinct pairs with count >= best - 16  hit     the merged bytes were a token already
      pair    (left bytes, right bytes)               apart   the merge shares no token with the merge in front of it
    (16 = KMAX: the least distance under the top the selection's first window reaches down.)"""
    known = set(base_tokens(specials))
    words = [[bytes([b]) for b in w] for w in types]
    steps: list[dict] = []
    prev: tuple[bytes, bytes] | None = None
    while len(steps) < num_merges:
        pc: Counter = Counter()
        for w, f in zip(words, freqs):
            for j in range(len(w) - 1):
                pc[(w[j], w[j + 1])] += int(f)
        if not pc:
            break
        best, cnt = max(pc.items(), key=lambda kv: (kv[1], kv[0]))
        if cnt < min_frequency:
            break
        x, y = best
        z = x + y
        steps.append({"count": cnt, "at_top": sum(1 for v in pc.values() if v == cnt), "near": sum(1 for v in pc.values() if v + 16 >= cnt),
                      "hit": z in known, "pair": best, "apart": prev is not None and not ({x, y} & set(prev))})
        known.add(z)
        prev = best
        for w in words:
            j = 0
            while j + 1 < len(w):
                if w[j] == x and w[j + 1] == y:
                    w[j:j + 2] = [z]
                j += 1
    return steps
