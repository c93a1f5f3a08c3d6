"""GPU: BBPETokenizer.repetition_array (yabpe_repetition) against the plain-Python repetition_stats -- top, distinct, covered
and every integer statistic, exactly: the hand-built documents of rep_helpers.py at three sets of lengths, through the LDS form
and with every document forced through the table in HBM; that table forced to a load near 1; 0 and 1 documents;
yabpe_encode's device results passed straight in; each error code."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import mask_helpers, rep_helpers as rh
from yet_another_bpe import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mask_helpers.tokenizer()


@functools.lru_cache(maxsize=None)
def expected(ngrams):
    return mask_helpers.tokenizer().repetition_stats(rh.corpus(), ngrams=ngrams)


def check(tok, docs, ngrams, exp=None, boundary=_native.REP_DOC, n_slots=None):
    exp = exp or tok.repetition_stats(docs, ngrams=ngrams)
    top, distinct, covered, st = tok.repetition_array(*rh.flat(docs), ngrams=ngrams)
    exp_st = rh.integer_stats(docs, ngrams, boundary)
    exp_st["n_slots"] = exp_st["n_slots"] if n_slots is None else n_slots
    print(ngrams, exp_st, st)
    for got, want in zip((top, distinct, covered), exp):
        assert got.dtype == np.uint32 and got.shape == (len(docs), len(ngrams)) and got.tolist() == want
    assert {k: st[k] for k in exp_st} == exp_st
    return st


@pytest.mark.parametrize("doc_max", [0, 1], ids=["lds", "all-long"])
@pytest.mark.parametrize("ngrams", rh.NGRAM_SETS)
def test_signals_match_plain_python(tok, ngrams, doc_max):
    """doc_max 1: every document of two ids or more takes the long form -- the same results"""
    ctx = tok._device()
    ctx.set_option("rep_doc_max", doc_max)
    try:
        st = check(tok, rh.corpus(), ngrams, expected(ngrams), boundary=doc_max or _native.REP_DOC)
        assert st["n_long_docs"] == (17 if doc_max else 2)  # (20 documents, three of them of 0 or 1 ids)
    finally:
        ctx.set_option("rep_doc_max", 0)


def test_long_form_table_at_a_load_near_one(tok):
    """1,023 windows of 5 random 32-bit ids in a table forced to 2^10 slots: unequal windows share chains of hundreds of slots
    that wrap the table's end; 1,024 windows need one slot more and are refused."""
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, 1 << 32, k, dtype=np.uint64).tolist() for k in (0, 300, 5, 411, 3, 323)]  # 296 + 1 + 407 + 319 windows
    docs[3][100:112], docs[5][300:310] = docs[1][20:32], docs[5][10:20]  # across documents: unseen; inside one: counted
    ctx = tok._device()
    ctx.set_option("rep_doc_max", 1)
    ctx.set_option("rep_slots_log2", 10)
    try:
        st = check(tok, docs, (5, 7), boundary=1, n_slots=1 << 10)
        assert st["n_long_windows"] == 1023 + (294 + 405 + 317)
        docs[5].append(7)  # 1,024 windows: windows + 1 slots are needed
        with pytest.raises(_native.YabpeError) as e:
            tok.repetition_array(*rh.flat(docs), ngrams=(5, 7))
        assert e.value.code == _native.E_INVALID
    finally:
        ctx.set_option("rep_doc_max", 0)
        ctx.set_option("rep_slots_log2", 0)


def test_no_document_and_one_document(tok):
    for docs in ([], [[]], [[3, 3, 3, 3, 3]]):
        check(tok, docs, (2, 3))


def test_encode_device_results_go_straight_in_and_stay(tok):
    docs = mask_helpers.word_docs()[:40]
    docs = docs + ["again " + docs[6] + " and " + docs[6], docs[9] * 3]  # (documents repeated inside themselves)
    exp_ids, *exp = tok.encode_batch_repetition(docs)
    ids, off, *got = tok.encode_array_repetition(docs)
    assert ids.tolist() == [t for d in exp_ids for t in d] and off.tolist() == [0] + np.cumsum([len(d) for d in exp_ids]).tolist()
    assert [g.tolist() for g in got] == exp and max(exp[2][-2]) > 100
    ctx = tok._device()
    di, dd, ni = ctx.encode("".join(docs).encode(), None, np.cumsum([0] + [len(d.encode()) for d in docs[:-1]]).astype(np.uint64))
    again = ctx.repetition_to_host(di, ni, dd, len(docs))  # (yabpe_encode's buffers: read, and left as they were)
    assert [g.tolist() for g in again] == exp
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), ids) and np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), off)
    assert [x.shape for x in tok.encode_array_repetition([])] == [(0,), (1,), (0, 9), (0, 9), (0, 9)]


@pytest.mark.parametrize("code, ids, starts, kw", [
    (_native.E_INVALID, [1, 2], [0], {"ngrams": ()}), (_native.E_INVALID, [1, 2], [0], {"ngrams": tuple(range(1, 18))}),
    (_native.E_INVALID, [1, 2], [0], {"ngrams": (0,)}), (_native.E_INVALID, [1, 2], [0], {"ngrams": (65,)}),
    (_native.E_INVALID, [1, 2], [0], {"ngrams": (2, 2)}), (_native.E_INVALID, [1, 2], [0], {"ngrams": (3, 2)}),
    (_native.E_INVALID, [1, 2], [0], {"flags": 1}), (_native.E_INVALID, [1, 2], [1], {}), (_native.E_INVALID, [1, 2], [0, 3], {}),
    (_native.E_INVALID, [1, 2], [0, 2, 1], {}), (_native.E_INVALID, [1, 2], [], {}), (_native.E_CAPACITY, 0, [0], {"n_ids": (1 << 30) + 1})])
def test_error_codes(tok, code, ids, starts, kw):
    """(the capacity case is refused before anything is read: its ids are never looked at)"""
    kw = dict(kw)
    with pytest.raises(_native.YabpeError) as e:
        tok._device().repetition(ids, kw.pop("n_ids", None), starts, **kw)
    assert e.value.code == code
