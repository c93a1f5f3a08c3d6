"""Helpers of the resume tests: the literal replay (the specification of the state a resumed load restores), a naive BPE
continuation from segmented words, and the CPU model of the device's word walk (tests/hostmodel/replay_model.cpp)."""
from __future__ import annotations

import ctypes
import subprocess
from collections import Counter, defaultdict
from pathlib import Path

import numpy as np

from tests import helpers
from yet_another_bpe import _native

HM = Path(__file__).resolve().parent / "hostmodel"


def replace_pair(word: tuple, left: bytes, right: bytes) -> tuple:
    """Greedy left-to-right, non-overlapping (trainer.py:276-285)."""
    out, i, n = [], 0, len(word)
    while i < n:
        if i + 1 < n and word[i] == left and word[i + 1] == right:
            out.append(left + right)
            i += 2
        else:
            out.append(word[i])
            i += 1
    return tuple(out)


def literal_replay(word: bytes, merges) -> tuple:
    """The word as the training loop leaves it: rewritten by merge 0, then merge 1, ... (tokens as byte strings: one id per
    byte string, so this is the replay over id pairs)."""
    w = tuple(bytes([b]) for b in word)
    for left, right in merges:
        if len(w) < 2:
            break
        if left in w:  # (otherwise replace_pair returns w as it is)
            w = replace_pair(w, left, right)
    return w


def tokenizer_rule(word: bytes, merges) -> tuple:
    """BBPETokenizer's rule: repeatedly the adjacent pair of lowest rank, leftmost on ties, keyed by bytes, the LAST index of
    a duplicated pair being its rank."""
    rank = {pair: i for i, pair in enumerate(merges)}
    w = [bytes([b]) for b in word]
    while len(w) > 1:
        best = min(range(len(w) - 1), key=lambda i: (rank.get((w[i], w[i + 1]), len(merges)), i))
        if (w[best], w[best + 1]) not in rank:
            break
        w[best:best + 2] = [w[best] + w[best + 1]]
    return tuple(w)


def naive_continue(segmented: dict, vocab: dict, budget: int, min_frequency: int):
    """A plain BPE loop from words that are already segmented: `segmented` {tuple of byte strings: frequency}, `vocab`
    {bytes: id}.  Counts from the words, max by (count, (left bytes, right bytes)) (trainer.py:246), greedy replacement, the
    merged bytes get the next id unless they are a token already; at most `budget` iterations.
    -> (vocab, new merges)."""
    vocab = dict(vocab)
    freq_of: dict[tuple, int] = defaultdict(int)
    for w, f in segmented.items():
        freq_of[tuple(w)] += f
    count_of: dict[tuple, int] = defaultdict(int)
    words_with: dict[tuple, set] = defaultdict(set)
    for w, f in freq_of.items():
        for pair in zip(w, w[1:]):
            count_of[pair] += f
            words_with[pair].add(w)
    merges = []
    for _ in range(max(0, budget)):
        live = [(c, p) for p, c in count_of.items() if c > 0]
        if not live:
            break
        cnt, best = max(live)
        if cnt < min_frequency:
            break
        for w in list(words_with.pop(best, ())):
            f = freq_of.pop(w, 0)
            if not f:
                continue
            for pair in zip(w, w[1:]):
                count_of[pair] -= f
                words_with[pair].discard(w)
            nw = replace_pair(w, *best)
            freq_of[nw] += f
            for pair in zip(nw, nw[1:]):
                count_of[pair] += f
                words_with[pair].add(nw)
        count_of.pop(best, None)
        merges.append(best)
        if best[0] + best[1] not in vocab:
            vocab[best[0] + best[1]] = len(vocab)
    return vocab, merges


def resume_naive(words, base, merges, budget: int, min_frequency: int):
    """Literal replay of `merges` over the pooled `words`, then the naive continuation: -> (vocab, all merges)."""
    toks, _ = _native.merge_triples(base, merges)
    seg: dict[tuple, int] = defaultdict(int)
    for w, f in Counter(bytes(w) for w in words).items():
        seg[literal_replay(w, merges)] += f
    vocab, new = naive_continue(seg, {t: i for i, t in enumerate(toks)}, budget, min_frequency)
    return vocab, list(merges) + new


def resumed_train(words, freq, base, merges, budget, min_frequency, dedup=False, check=True, options=None):
    """-> (vocab, all merges, resume stats, stats) of a fresh context that continues from (base, merges) on the pooled words
    (GPU).  options: yabpe_set_option pairs set before the vocabulary (id_bits = 32: the u32 resumed load)."""
    toks, triples = _native.merge_triples(base, merges)
    flat, off = helpers.flatten(words)
    with _native.Context() as ctx:
        for k, v in (options or {}).items():
            ctx.set_option(k, v)
        ctx.set_vocab(toks)
        ctx.load_words_resumed(flat, off, freq, triples, dedup=dedup)
        if check:
            assert ctx.verify_table() == 0
        left, right, merged, _count = ctx.train(budget, min_frequency)
        if check:
            assert ctx.verify_table() == 0
        rs, st = ctx.resume_stats(), ctx.stats()
    vocab, new = _native.decode_merges(toks, left, right, merged)
    return vocab, list(merges) + new, rs, st


# ---------------------------------------------------------------- the CPU model of the device's walk
def replay_lib():
    so, src = HM / "libreplay_model.so", HM / "replay_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "replay_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.replay_model.restype = ctypes.c_int
    lib.replay_model_lookup.restype = ctypes.c_int
    lib.replay_model_lookup32.restype = ctypes.c_int
    return lib


def model_replay(lib, words, triples, form: int) -> list[list[int]]:
    """The CPU model's tokens (ids) of every word.  form 0: sequential walk, 1: lane form up to 64 bytes."""
    left, right, merged = (np.ascontiguousarray(x, dtype=np.uint32) for x in triples)
    data = b"".join(words)
    flat = np.frombuffer(data or b"\0", dtype=np.uint8).copy()
    off = np.zeros(len(words) + 1, dtype=np.uint64)
    np.cumsum([len(w) for w in words], out=off[1:])
    out = np.zeros(len(data) + 1, dtype=np.uint16)
    cnt = np.zeros(len(words) + 1, dtype=np.uint32)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.replay_model(vp(left), vp(right), vp(merged), ctypes.c_uint32(len(left)), vp(flat), vp(off), ctypes.c_uint64(len(words)),
                          ctypes.c_int(form), vp(out), vp(cnt))
    assert rc == 0
    o = off.tolist()
    return [out[o[i]:o[i] + int(cnt[i])].tolist() for i in range(len(words))]


def model_lookup32(lib, triples, queries):
    """The table at 64-bit keys, built by the shared builder from `triples`, asked `queries` = [(a, b, tmin)]: a list of
    (rank, merged) or None per query, then the number of index keys away from their hash's slot and of those that wrapped."""
    left, right, merged = (np.ascontiguousarray(x, dtype=np.uint32) for x in triples)
    q = np.array(queries, dtype=np.uint32).reshape(-1, 3)
    a, b, tmin = (np.ascontiguousarray(q[:, k]) for k in range(3))
    found = np.zeros(len(q) + 1, dtype=np.uint8)
    rank, res = np.zeros(len(q) + 1, dtype=np.uint32), np.zeros(len(q) + 1, dtype=np.uint32)
    displaced, wrapped = ctypes.c_uint32(0), ctypes.c_uint32(0)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.replay_model_lookup32(vp(left), vp(right), vp(merged), ctypes.c_uint32(len(left)), vp(a), vp(b), vp(tmin), ctypes.c_uint32(len(q)),
                                   vp(found), vp(rank), vp(res), ctypes.byref(displaced), ctypes.byref(wrapped))
    assert rc == 0
    return [(int(rank[i]), int(res[i])) if found[i] else None for i in range(len(q))], displaced.value, wrapped.value
