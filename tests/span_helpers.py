"""Shared by the span-corruption tests, CPU and GPU: the case list both the CPU model (tests/hostmodel/span_model.cpp) and
yabpe_span_corrupt run against the plain-Python BBPETokenizer.corrupt_spans, on the synthetic ids of tests/mask_helpers.py
(ids below 1000, so an id of SENT_BASE or more in a result is a sentinel).  A case carries raw thresholds (To, C), as the C ABI
takes them; the plain Python gets the same integers through its span_thresholds.  Cases that claim a situation -- a span over
a block edge, an opener just before one, a span at a document's end -- find their seed by a search over the rule's own
draws and carry a predicate that test_span_model.py asserts, so a change of the rule cannot leave them testing nothing."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from tests import mask_helpers as mh
from yet_another_bpe.synth import rnd_int
from yet_another_bpe.tokenizer import BBPETokenizer

SENT_BASE = 9000
ONE = 1 << 32


def sentinels(n: int) -> list[int]:
    return list(range(SENT_BASE, SENT_BASE + n))


@lru_cache(maxsize=None)
def thresholds(p, mean, lmax) -> tuple[int, tuple[int, ...]]:
    To, C = BBPETokenizer.span_thresholds(p, mean, lmax)
    return To, tuple(C)


def reaches(seed: int, first_doc: int, d: int, To: int, C, n: int) -> list[int]:
    """per unit u < n of document d: one past the last unit its span covers, u itself if it does not open -- the rule's
    definition, written out once more"""
    kd = rnd_int(seed, 0x63, first_doc + d)
    out = []
    for u in range(n):
        r = rnd_int(kd, 0x6f, u)
        out.append(u + 1 + sum((r & 0xFFFFFFFF) < c for c in C) if (r >> 32) < To else u)
    return out


def noise_of(reach: list[int], lmax: int) -> list[bool]:
    return [any(reach[u] > v for u in range(max(0, v - lmax + 1), v + 1)) for v in range(len(reach))]


def find_seed(lens, To, C, pred, first_doc: int = 0) -> int:
    """the first seed whose draws (token mode) satisfy pred(reach per document, noise per document)"""
    for seed in range(2000):
        reach = [reaches(seed, first_doc, d, To, C, n) for d, n in enumerate(lens)]
        if pred(reach, [noise_of(r, len(C) + 1) for r in reach]):
            return seed
    raise AssertionError("no seed in 0 .. 1999 gives the situation")


def _case(name, lens, *, To, C, seed=0, first_doc=0, with_off=True, words="none", whole_word=False, n_sent=100, final=True, cut=0, pred=None,
          batch_seed=1, special=None):
    """words: "none" (no words array), "given" (words and specials of the synthetic batch) -- whole_word needs "given".
    special: per-document lists that replace the synthetic batch's."""
    return {"name": name, "lens": list(lens), "To": To, "C": tuple(C), "seed": seed, "first_doc": first_doc, "with_off": with_off, "words": words,
            "whole_word": whole_word, "n_sent": n_sent, "final": final, "cut": cut, "pred": pred, "batch_seed": batch_seed, "special": special}


@lru_cache(maxsize=None)
def cases() -> tuple[dict, ...]:
    out = []
    T15, T50 = thresholds(0.15, 3.0, 10), thresholds(0.5, 3.0, 10)
    # the document sets of the mask tests: empty documents at both ends and in the middle, 600 one-token documents, a 700-token
    # document, no ids, no doc_off, a block edge at a document edge -- per token, per token with specials, per word
    for k, (name, lens, with_off) in enumerate(mh.LENGTH_SETS):
        for (To, C), (words, whole_word), (seed, first_doc) in (
                (T15, ("none", False), (0, 0)), (T50, ("given", False), (12345, 1 << 40)), (T50, ("given", True), (k, 0)), (T15, ("given", True), (7, 3))):
            out.append(_case(f"{name}; To {To} {words} whole_word {whole_word}", lens, To=To, C=C, seed=seed, first_doc=first_doc, with_off=with_off,
                             words=words, whole_word=whole_word))
    long5 = [3, 3, 700, 3, 3]  # the long document starts at id 6: blocks end after its tokens 249 and 505
    To, C = T50
    edges = lambda reach, noise: noise[2][249] and noise[2][250] and noise[2][505] and noise[2][506]  # noqa: E731
    out.append(_case("runs across both block edges of a 700-token document", long5, To=To, C=C, seed=find_seed(long5, To, C, edges), pred=edges))
    To, C = T15
    opener = lambda reach, noise: (reach[0][256] == 256 and noise[0][256] and not any(reach[0][u] > 256 for u in range(247, 254))  # noqa: E731
                                   and reach[0][254] <= 254)  # only unit 255, the block's last id, reaches id 256
    out.append(_case("an opener on the last id of a block covers the next block's first", [700], To=To, C=C, seed=find_seed([700], To, C, opener), pred=opener))
    far = lambda reach, noise: (reach[0][250] > 256 and not any(reach[0][u] > u for u in range(251, 257))  # noqa: E731
                                and not any(reach[0][u] > 256 for u in range(247, 250)))
    out.append(_case("an opener six ids before a block edge covers the id past it", [700], To=To, C=C, seed=find_seed([700], To, C, far), pred=far))
    at_end = lambda reach, noise: reach[0][4] >= 7 and not noise[1][0] and not noise[1][1]  # noqa: E731
    out.append(_case("a span that would cross its document's end stops there", [5, 5], To=To, C=C, seed=find_seed([5, 5], To, C, at_end), pred=at_end))
    clipped = lambda reach, noise: reach[0][0] >= 3 and reach[0][1] == 1 and reach[0][2] == 2  # noqa: E731
    out.append(_case("look-back clipped at the document's first token", [4, 2, 1], To=To, C=C, seed=find_seed([4, 2, 1], To, C, clipped), pred=clipped))
    # a special inside a covered stretch: two runs, two sentinels (To = 2^32: every unit opens)
    out.append(_case("a special splits a covered stretch", [6, 3], To=ONE, C=T15[1], words="given", special=[[False, False, False, True, False, False], [True, False, True]]))
    out.append(_case("a special splits a covered stretch, whole words", [6, 3], To=ONE, C=T15[1], words="given", whole_word=True,
                     special=[[False, False, False, True, False, False], [True, False, True]]))
    # the cut inside a run and on a run start (the second document is shorter than either cut)
    To, C = T50
    two = [60, 9]
    seed = find_seed(two, To, C, lambda reach, noise: any(noise[0][j - 1] and noise[0][j] for j in range(12, 50)))
    noise = noise_of(reaches(seed, 0, 0, To, C, 60), 10)
    inside = next(j for j in range(12, 50) if noise[j - 1] and noise[j])
    on_start = next(j for j in range(12, 50) if not noise[j - 1] and noise[j])
    out.append(_case("the cut inside a run", two, To=To, C=C, seed=seed, cut=inside, pred=lambda reach, n, j=inside: n[0][j - 1] and n[0][j]))
    out.append(_case("the cut on a run start", two, To=To, C=C, seed=seed, cut=on_start, pred=lambda reach, n, j=on_start: not n[0][j - 1] and n[0][j]))
    out.append(_case("the cut, whole words and specials", [300, 0, 40, 2], To=To, C=C, seed=3, cut=37, words="given", whole_word=True))
    out.append(_case("a cut of one token", [5, 0, 1, 300], To=To, C=C, seed=4, cut=1))
    # the sentinel cap on documents with more than three runs
    many = lambda reach, noise: all(sum(n[j] and not (j and n[j - 1]) for j in range(len(n))) > 3 for n in noise)  # noqa: E731
    for n_sent in (2, 3):
        for final in (True, False):
            out.append(_case(f"{n_sent} sentinels, final {final}: runs past the cap stay", [200, 300], To=To, C=C, seed=5, n_sent=n_sent, final=final, pred=many))
    out.append(_case("one sentinel and no final one", [200, 0, 2], To=To, C=C, seed=6, n_sent=1, final=False))
    out.append(_case("the cap, whole words, specials and the cut", [200, 300], To=To, C=C, seed=8, n_sent=3, words="given", whole_word=True, cut=150))
    # Lmax = 1 and 32
    out.append(_case("Lmax 1", long5, To=thresholds(0.3, 3.0, 1)[0], C=(), seed=9))
    out.append(_case("Lmax 32", long5, To=thresholds(0.3, 8.0, 32)[0], C=thresholds(0.3, 8.0, 32)[1], seed=10))
    out.append(_case("Lmax 32, whole words", long5, To=thresholds(0.3, 8.0, 32)[0], C=thresholds(0.3, 8.0, 32)[1], seed=11, words="given", whole_word=True))
    out.append(_case("Lmax 32, every length threshold 2^32", [100, 3], To=thresholds(0.05, 3.0, 10)[0], C=(ONE,) * 31, seed=12))
    # To = 0 and To = 2^32
    for To in (0, ONE):
        out.append(_case(f"To {To}", mh.LENGTH_SETS[0][1], To=To, C=T15[1], words="given", seed=13))
        out.append(_case(f"To {To}, no words, final False", long5, To=To, C=T15[1], seed=14, final=False))
    out.append(_case("To 2^32, one document without doc_off", [515], To=ONE, C=T15[1], with_off=False, n_sent=2))
    return tuple(out)


CASE_IDS = [c["name"] for c in cases()]


@lru_cache(maxsize=None)
def batch(index: int):
    """-> (ids_batch, words_batch or None, special_batch or None) of case `index`"""
    c = cases()[index]
    ids_b, words_b, special_b = mh.synth_batch(c["lens"], seed=c["batch_seed"])
    if c["special"] is not None:
        special_b = c["special"]
    return (ids_b, words_b, special_b) if c["words"] == "given" else (ids_b, None, None)


def python_result(ids_b, words_b, special_b, c, n_sent=None):
    """corrupt_spans with the case's integers: the tokenizer's span_thresholds is replaced by one that returns them"""
    tok = BBPETokenizer()
    tok.span_thresholds = lambda p, mean, lmax: (c["To"], list(c["C"]))
    return tok.corrupt_spans(ids_b, words_b, special_b, sentinels=sentinels(n_sent or c["n_sent"]), seed=c["seed"], first_doc=c["first_doc"],
                             whole_word=c["whole_word"], final_sentinel=c["final"], max_tokens=c["cut"] or None)


@lru_cache(maxsize=None)
def expected(index: int):
    """-> (inputs, targets, counts) of case `index` from the plain Python, computed once.  counts: what yabpe_span_stats
    reports, taken from this result and from one with a sentinel for every run (ids are below SENT_BASE)."""
    c = cases()[index]
    ids_b, words_b, special_b = batch(index)
    inputs, targets = python_result(ids_b, words_b, special_b, c)
    free_in, _free_tgt = python_result(ids_b, words_b, special_b, c, n_sent=max(c["lens"], default=0) + 2)
    kept = [min(n, c["cut"]) if c["cut"] else n for n in c["lens"]]
    runs = sum(x >= SENT_BASE for row in free_in for x in row)
    counts = {"n_ids": sum(c["lens"]), "n_docs": max(len(c["lens"]), 1),
              "n_protected": sum(sum(s) for s in special_b) if special_b is not None else 0,
              "n_noise": sum(kept) - (sum(len(r) for r in free_in) - runs), "n_runs": runs,
              "n_runs_over": runs - sum(x >= SENT_BASE for row in inputs for x in row), "n_cut": sum(c["lens"]) - sum(kept),
              "n_in": sum(len(r) for r in inputs), "n_tgt": sum(len(r) for r in targets)}
    return inputs, targets, counts


def flat_arrays(index: int):
    """-> (ids u32, document starts u64 or None, packed words u32 or None) of case `index`, as the C ABI takes them"""
    c = cases()[index]
    ids_b, words_b, special_b = batch(index)
    return (mh.flat(ids_b, np.uint32), mh.starts(c["lens"]) if c["with_off"] else None,
            mh.packed_words(words_b, special_b) if words_b is not None else None)


def ragged(flat, off) -> list[list[int]]:
    flat, off = np.asarray(flat).tolist(), np.asarray(off).tolist()
    return [flat[off[d]:off[d + 1]] for d in range(len(off) - 1)]
