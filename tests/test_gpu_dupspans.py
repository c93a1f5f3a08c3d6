"""GPU: BBPETokenizer.duplicate_spans_array (yabpe_dup_spans) against the plain-Python duplicate_spans -- masks, n_dup, the
compacted ids / offsets and every integer statistic, exactly: the hand-built corpora of dup_helpers.py at every min_len; a table
forced to a load near 1; 0 and 1 documents; yabpe_encode's device results passed straight in; encode_array_dedup against
encode_batch_dedup and through decode_array; each error code."""
from __future__ import annotations

import numpy as np
import pytest

from tests import dup_helpers as dh, mask_helpers
from yet_another_bpe import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mask_helpers.tokenizer()


def check(tok, docs, n):
    masks, n_dup, exp_st = tok.duplicate_spans(docs, min_len=n)
    ids, off = dh.flat(docs)
    dup, got_n, st, kept, kept_off = tok.duplicate_spans_array(ids, off, min_len=n, compact=True)
    print(n, exp_st, {k: st[k] for k in exp_st}, st["n_slots"])
    assert dup.dtype == np.uint8 and dup.tolist() == [m for mk in masks for m in mk] and got_n.tolist() == n_dup
    assert {k: st[k] for k in exp_st} == exp_st
    assert kept.dtype == np.uint32 and np.array_equal(kept, ids[dup == 0])
    assert kept_off.tolist() == [0] + np.cumsum([len(d) - k for d, k in zip(docs, n_dup)]).tolist()
    plain = tok.duplicate_spans_array(ids, off, min_len=n)  # (without the flag: the same mask, nothing else)
    assert len(plain) == 3 and np.array_equal(plain[0], dup) and np.array_equal(plain[1], got_n)
    return st


@pytest.mark.parametrize("n", dh.MIN_LENS)
@pytest.mark.parametrize("name", dh.CORPORA)
def test_spans_match_plain_python(tok, name, n):
    st = check(tok, dh.corpus(name, n), n)
    assert st["n_slots"] == max(1 << 10, 1 << max(2 * st["n_windows"] - 1, 0).bit_length())


def test_table_at_a_load_near_one(tok):
    """1,023 windows of 5 random 32-bit ids, 1,009 of them distinct, in a table forced to 2^10 slots (load 0.985): unequal
    windows share chains of hundreds of slots that wrap the table's end; 1,024 windows need one slot more and are refused."""
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, 1 << 32, k, dtype=np.uint64).tolist() for k in (0, 300, 5, 411, 3, 323)]  # 296 + 1 + 407 + 319 windows
    docs[3][100:112], docs[5][300:310] = docs[1][20:32], docs[5][10:20]  # the repeats: across documents, inside one
    ctx = tok._device()
    ctx.set_option("dup_slots_log2", 10)
    try:
        st = check(tok, docs, 5)
        assert (st["n_slots"], st["n_windows"], st["n_repeats"]) == (1 << 10, 1023, 14)
        docs[5].append(7)  # 1,024 windows: windows + 1 slots are needed
        with pytest.raises(_native.YabpeError) as e:
            tok.duplicate_spans_array(*dh.flat(docs), min_len=5)
        assert e.value.code == _native.E_INVALID
    finally:
        ctx.set_option("dup_slots_log2", 0)


def test_no_document_and_one_document(tok):
    for docs in ([], [[]], [[3, 3, 3, 3, 3]]):
        st = check(tok, docs, 2)
        assert (st["n_docs"], st["n_dup_ids"]) == (len(docs), 3 if docs and docs[0] else 0)


def test_encode_device_results_go_straight_in_and_stay(tok):
    docs = mask_helpers.word_docs()[:40]
    docs = docs + ["again " + docs[6] + " and the end"] + docs[8:14]  # (the long document and short ones, repeated)
    exp, exp_n = tok.encode_batch_dedup(docs, min_len=8)
    ids, off, n_dup = tok.encode_array_dedup(docs, min_len=8)
    assert n_dup.tolist() == exp_n and sum(exp_n) > 700 and ids.tolist() == [t for d in exp for t in d]
    assert off.tolist() == [0] + np.cumsum([len(d) for d in exp]).tolist()
    text, text_off = tok.decode_array(ids, off)
    assert [bytes(text[text_off[d]:text_off[d + 1]]).decode() for d in range(len(docs))] == [tok.decode(d) for d in exp]
    ctx = tok._device()
    all_ids, all_off = tok.encode_array(docs)
    di, dd, ni = ctx.encode("".join(docs).encode(), None, np.cumsum([0] + [len(d.encode()) for d in docs[:-1]]).astype(np.uint64))
    dup, got_n, kept, kept_off = ctx.dup_spans_to_host(di, ni, dd, len(docs), min_len=8, compact=True)  # (yabpe_encode's buffers)
    assert got_n.tolist() == exp_n and np.array_equal(kept, ids) and np.array_equal(kept_off, off)
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), all_ids) and np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), all_off)
    assert [x.shape for x in tok.encode_array_dedup([])] == [(0,), (1,), (0,)]


@pytest.mark.parametrize("code, ids, starts, kw", [
    (_native.E_INVALID, [1, 2], [0], {"min_len": 0}), (_native.E_INVALID, [1, 2], [0], {"min_len": 1025}),
    (_native.E_INVALID, [1, 2], [0], {"min_len": 2, "flags": 2}), (_native.E_INVALID, [1, 2], [1], {}), (_native.E_INVALID, [1, 2], [0, 3], {}),
    (_native.E_INVALID, [1, 2], [0, 2, 1], {}), (_native.E_INVALID, [1, 2], [], {}), (_native.E_CAPACITY, 0, [0], {"n_ids": (1 << 30) + 1})])
def test_error_codes(tok, code, ids, starts, kw):
    """(the capacity case is refused before anything is read: its ids are never looked at)"""
    kw = dict(kw)
    with pytest.raises(_native.YabpeError) as e:
        tok._device().dup_spans(ids, kw.pop("n_ids", None), starts, **kw)
    assert e.value.code == code
