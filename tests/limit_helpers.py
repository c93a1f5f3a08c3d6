"""An independent plain-Python BPE trainer with a maximum token length, the model the limit tests compare with.

No incremental state: at every step all pairs are recounted from the words as they are segmented now, the pairs whose two
tokens are together longer than the limit are filtered out, the maximum by (count, (left bytes, right bytes)) is taken and
every word is rewritten.  It shares nothing with the device's tables, deltas or selection.

Tokens are `bytes`, a word is a tuple of tokens; Python's ordering of (bytes, bytes) tuples is the tie-break.
"""
from __future__ import annotations

from functools import lru_cache

from tests import helpers

SP = ["<|endoftext|>"]


def _rewrite(word: tuple, left: bytes, right: bytes) -> tuple:
    """Greedy left-to-right, non-overlapping replacement of (left, right) by left + right."""
    if left not in word:
        return word
    out = []
    i, n = 0, len(word)
    while i < n:
        if i + 1 < n and word[i] == left and word[i + 1] == right:
            out.append(left + right)
            i += 2
        else:
            out.append(word[i])
            i += 1
    return tuple(out)


def segment(words, merges):
    """Every word as single bytes, then every merge of `merges` applied in order: the state a resumed job starts from."""
    segs = [tuple(bytes([b]) for b in w) for w in words]
    for left, right in merges:
        segs = [_rewrite(s, left, right) for s in segs]
    return segs


def train(words, freq, num_merges, min_frequency, specials, limit=None, start_merges=(), trace=None):
    """words: byte strings (repeats allowed), freq: their counts or None (1 each).  Returns (vocab {bytes: id}, merges): the
    merges learned here, after `start_merges` have been replayed as they are (their tokens get their ids first, and are not
    subject to the limit).  limit: None, or the largest len(left) + len(right) a learned merge may have.
    trace (a dict, optional) receives why the loop ended: "stop" in {"cap", "no_pairs", "min_frequency"}, and for the last look
    at the counts "best_eligible" / "best_ineligible" (the highest count on either side of the limit, 0 when there is none)."""
    vocab = {t: i for i, t in enumerate(helpers.base_tokens(specials))}
    for left, right in start_merges:
        vocab.setdefault(left + right, len(vocab))
    pooled: dict[tuple, int] = {}
    counts = [1] * len(words) if freq is None else [int(f) for f in freq]
    for seg, f in zip(segment(words, start_merges), counts):
        pooled[seg] = pooled.get(seg, 0) + f
    merges = []
    why = "cap"
    info = {"best_eligible": 0, "best_ineligible": 0}
    while len(merges) < num_merges:
        pairs: dict[tuple, int] = {}
        for seg, f in pooled.items():
            for pair in zip(seg, seg[1:]):
                pairs[pair] = pairs.get(pair, 0) + f
        ok = {p: c for p, c in pairs.items() if limit is None or len(p[0]) + len(p[1]) <= limit}
        info = {"best_eligible": max(ok.values(), default=0),
                "best_ineligible": max((c for p, c in pairs.items() if p not in ok), default=0)}
        if not ok:
            why = "no_pairs"
            break
        count, (left, right) = max((c, p) for p, c in ok.items())
        if count < min_frequency:
            why = "min_frequency"
            break
        merges.append((left, right))
        vocab.setdefault(left + right, len(vocab))
        again: dict[tuple, int] = {}
        for seg, f in pooled.items():
            seg = _rewrite(seg, left, right)
            again[seg] = again.get(seg, 0) + f
        pooled = again
    if trace is not None:
        trace.update(info, stop=why)
    return vocab, merges


# ---------------------------------------------------------------- the shared input of the limit tests
N_WORDS = 6000  # the first pre-tokens of corpus.en


@lru_cache(maxsize=None)
def en_words() -> tuple:
    return tuple(helpers.corpus_en_words()[:N_WORDS])


@lru_cache(maxsize=None)
def en_model(limit, num_merges=400, min_frequency=2):
    """(vocab, merges, trace) of the helper on the 6,000 pre-tokens; computed once per argument set and shared."""
    uw, fq = helpers.pooled(en_words())
    trace: dict = {}
    vocab, merges = train(uw, fq, num_merges, min_frequency, SP, limit=limit, trace=trace)
    return vocab, merges, trace


def first_difference(a, b) -> int:
    """Index of the first merge at which two merge lists differ (the shorter one's length when one is a prefix)."""
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return min(len(a), len(b))
