"""Hand-built ragged id documents the repetition-signal tests share (test_gpu_repetition.py), and the integer statistics
yabpe_repetition reports, from the lengths alone."""
from __future__ import annotations

import numpy as np

from yet_another_bpe import _native

NGRAM_SETS = ((1,), (2, 3, 4, 5, 6, 7, 8, 9, 10), (64,))


def corpus(rep_doc: int = _native.REP_DOC) -> list:
    """-> the documents (lists of ids).  rep_doc: the short/long boundary the lengths are built around."""
    rng = np.random.default_rng(11)

    def rand(k):  # k ids, almost surely without a repeated window of any length
        return rng.integers(1000, 1 << 32, k, dtype=np.uint64).tolist()

    docs = [rand(k) for k in (0, 1, 2, 3, 9, 10, 11, 63, 64, 65)]  # 0, 1, and n - 1, n, n + 1 for n = 1, 2, 10, 64
    docs += [[7] * 130, ([1, 2, 3] * 50)[:140]]  # a run of one id; period 3
    same = rand(80)
    docs += [same, [], list(same)]  # identical, without internal repeats: they must not see each other
    far = rand(300)
    far[200:270] = far[10:80]  # one repeat far apart ...
    far[120:190] = (rand(7) * 10)[:70]  # ... and one that overlaps itself (period 7)
    docs.append(far)
    for L in (rep_doc - 1, rep_doc, rep_doc + 1):  # either side of the boundary between the forms; the repeat ends the document
        d = rand(L)
        d[L - 70:] = d[5:75]
        docs.append(d)
    seam = rand(2 * _native.DUP_TILE + 100)  # long form: the repeat's windows lie in the first piece and in the second
    seam[_native.DUP_TILE - 24:_native.DUP_TILE + 46] = seam[100:170]
    docs.append(seam)
    return docs


def flat(docs):
    """-> (ids np.uint32[n_ids], doc_off np.uint64[n_docs + 1])"""
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.asarray([t for d in docs for t in d], dtype=np.uint32), off


def integer_stats(docs, ngrams, boundary: int = _native.REP_DOC) -> dict:
    """what yabpe_repetition_stats holds for these documents: documents of more than `boundary` ids take the long form"""
    long_lens = [len(d) for d in docs if len(d) > boundary]
    windows = [sum(max(L - n + 1, 0) for L in long_lens) for n in ngrams]
    return {"n_ids": sum(len(d) for d in docs), "n_docs": len(docs), "n_ngrams": len(ngrams), "n_short_docs": len(docs) - len(long_lens),
            "n_long_docs": len(long_lens), "n_long_windows": sum(windows),
            "n_slots": max(1 << 10, 1 << max(2 * windows[0] - 1, 0).bit_length()) if long_lens else 0}
