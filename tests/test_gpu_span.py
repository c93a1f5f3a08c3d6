"""GPU: yabpe_span_corrupt bit for bit against the plain-Python BBPETokenizer.corrupt_spans on the cases of
tests/span_helpers.py (the list the CPU model runs), inputs as host arrays and as the device results of yabpe_encode_words,
with and without words, the call's statistics against counts taken from the Python result, results that outlive later
encode, mask and layout calls, yabpe_span_free and a second call, and every refused argument."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import mask_helpers as mh
from tests import span_helpers as sh

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


def native_args(c):
    return {"sentinels": np.asarray(sh.sentinels(c["n_sent"]), np.uint32), "seed": c["seed"], "first_doc": c["first_doc"], "open": c["To"],
            "lens": c["C"], "max_doc_ids": c["cut"], "whole_word": c["whole_word"], "final_sentinel": c["final"]}


@pytest.mark.parametrize("index", range(len(sh.cases())), ids=sh.CASE_IDS)
def test_matches_plain_python(tok, index):
    c = sh.cases()[index]
    exp_in, exp_tgt, counts = sh.expected(index)
    ids, starts, packed = sh.flat_arrays(index)
    ctx = tok._device()
    got_in, in_off, got_tgt, tgt_off = ctx.span_corrupt_to_host(ids, None, starts, None, packed, **native_args(c))
    assert (got_in.dtype, in_off.dtype, got_tgt.dtype, tgt_off.dtype) == (np.uint32, np.uint64, np.uint32, np.uint64)
    assert len(in_off) == len(tgt_off) == len(exp_in) + 1 and in_off[-1] == len(got_in) and tgt_off[-1] == len(got_tgt)
    assert sh.ragged(got_in, in_off) == exp_in and sh.ragged(got_tgt, tgt_off) == exp_tgt
    st = ctx.span_stats()
    assert {k: st[k] for k in counts} == counts
    if len(ids) and index % 4 == 0:  # the ids in device memory (a mask that selects nothing copies them there), the rest on the host
        d_ids, _labels = ctx.mask(ids, None, starts, None, None, select=0)
        again = ctx.span_corrupt_to_host(d_ids, len(ids), starts, None, packed, **native_args(c))
        assert all(np.array_equal(a, b) for a, b in zip(again, (got_in, in_off, got_tgt, tgt_off)))
        assert np.array_equal(ctx.d2h(d_ids, 4 * len(ids), np.uint32), ids)  # the inputs are left alone


def test_the_python_twin_takes_the_users_numbers(tok):
    lens = [3, 0, 400, 1, 1, 90]
    ids_b, words_b, special_b = mh.synth_batch(lens, seed=3)
    ids, words, special = mh.flat(ids_b, np.uint32), mh.flat(words_b, np.uint32), mh.flat(special_b, bool)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    for kw in ({"p": 0.15}, {"p": 0.5, "mean_span_length": 2.0, "max_span_length": 4, "whole_word": True, "seed": 9, "first_doc": 5},
               {"p": 0.3, "max_tokens": 50, "final_sentinel": False, "sentinels": sh.sentinels(3)}, {"p": 0}, {"p": 1}):
        kw = {"sentinels": sh.sentinels(100), **kw}
        exp_in, exp_tgt = tok.corrupt_spans(ids_b, words_b, special_b, **kw)
        got_in, in_off, got_tgt, tgt_off = tok.corrupt_spans_array(ids, off, words, special, **kw)
        assert sh.ragged(got_in, in_off) == exp_in and sh.ragged(got_tgt, tgt_off) == exp_tgt, kw
    kw = {"sentinels": sh.sentinels(100), "p": 0.4, "seed": 2}
    for words_arg, special_arg, wb, sb in ((None, None, None, None), (None, special, None, special_b)):  # no words; specials alone
        exp_in, exp_tgt = tok.corrupt_spans(ids_b, wb, sb, **kw)
        got_in, in_off, got_tgt, tgt_off = tok.corrupt_spans_array(ids, off, words_arg, special_arg, **kw)
        assert sh.ragged(got_in, in_off) == exp_in and sh.ragged(got_tgt, tgt_off) == exp_tgt
    assert tok._device().span_stats()["n_protected"] == int(special.sum())


def test_device_results_of_encode_words_go_straight_in(tok):
    docs = mh.word_docs()
    enc = tok.encode_batch_with_words(docs)
    ctx = tok._device()
    data, starts = tok._device_input(docs)
    sent = ["[MASK]", "[PAD]", "<|endoftext|>"]  # sentinels by string: specials that have ids
    To, C = sh.thresholds(0.3, 3.0, 10)
    for whole_word in (False, True):
        di, dd, dw, ni = ctx.encode_words(data, doc_starts=starts)
        before = [ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dw, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)]
        got_in, in_off, got_tgt, tgt_off = ctx.span_corrupt_to_host(di, ni, dd, len(docs), dw, sentinels=np.asarray(tok._sentinel_ids(sent), np.uint32),
                                                                    seed=4, first_doc=2, open=To, lens=C, whole_word=whole_word, final_sentinel=True)
        exp_in, exp_tgt = tok.corrupt_spans([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], sentinels=sent, p=0.3, seed=4,
                                            first_doc=2, whole_word=whole_word)
        assert sh.ragged(got_in, in_off) == exp_in and sh.ragged(got_tgt, tgt_off) == exp_tgt
        st = ctx.span_stats()
        assert st["n_protected"] == sum(sum(e[2]) for e in enc) > 0 and st["n_runs_over"] > 0 and st["n_cut"] == 0
        after = [ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dw, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_results_outlive_later_calls_and_a_second_call_replaces_them(tok):
    lens = [5, 0, 300, 2]
    ids_b, words_b, special_b = mh.synth_batch(lens, seed=5)
    ids, packed = mh.flat(ids_b, np.uint32), mh.packed_words(words_b, special_b)
    ctx = tok._device()
    To, C = sh.thresholds(0.5, 3.0, 10)
    kw = {"sentinels": np.asarray(sh.sentinels(100), np.uint32), "seed": 1, "open": To, "lens": C, "final_sentinel": True}
    di, dio, n_in, dt, dto, n_tgt, nd = ctx.span_corrupt(ids, None, mh.starts(lens), None, packed, **kw)

    def read():
        return (ctx.d2h(di, 4 * n_in, np.uint32), ctx.d2h(dio, 8 * (nd + 1), np.uint64), ctx.d2h(dt, 4 * n_tgt, np.uint32),
                ctx.d2h(dto, 8 * (nd + 1), np.uint64))

    first = read()
    rows, _lengths = ctx.layout_pad_to_host(di, n_in, dio, nd, row_len=16, pad_id=0)  # a layout call over the results ...
    tok.encode_array(mh.word_docs()[:20])
    tok.encode_array_padded(mh.word_docs()[:20], 16)
    tok.mask_array(ids, np.concatenate(([0], np.cumsum(lens))), mask_id=5000, n_random=7)
    assert all(np.array_equal(a, b) for a, b in zip(first, read()))  # ... and later calls leave them valid
    tok_py = type(tok)()
    exp_in, exp_tgt = tok_py.corrupt_spans(ids_b, None, special_b, sentinels=sh.sentinels(100), p=0.5, seed=1)
    assert sh.ragged(first[0], first[1]) == exp_in and sh.ragged(first[2], first[3]) == exp_tgt
    assert rows.tolist() == tok_py._padded_rows(exp_in, 16, 0, 0, None, None, "right", "right")[0]
    got = ctx.span_corrupt_to_host(ids, None, mh.starts(lens), None, packed, **{**kw, "seed": 2})  # a second call replaces them
    exp_in, exp_tgt = tok_py.corrupt_spans(ids_b, None, special_b, sentinels=sh.sentinels(100), p=0.5, seed=2)
    assert sh.ragged(got[0], got[1]) == exp_in and sh.ragged(got[2], got[3]) == exp_tgt
    ctx.span_free()
    ctx.span_free()
    got = ctx.span_corrupt_to_host(ids, None, mh.starts(lens), None, packed, **{**kw, "seed": 2})  # and after a free
    assert sh.ragged(got[0], got[1]) == exp_in


def test_refused_arguments(tok):
    from yet_another_bpe import _native

    ids = np.arange(10, dtype=np.uint32)
    ctx = tok._device()
    ok = {"sentinels": np.asarray(sh.sentinels(4), np.uint32), "open": 1 << 30, "lens": (1 << 31, 1 << 30), "final_sentinel": True}
    good = ctx.span_corrupt_to_host(ids, None, [0, 4], None, None, **ok)
    stats = ctx.span_stats()
    one, none = np.asarray(sh.sentinels(1), np.uint32), np.zeros(0, np.uint32)
    cases = [({"open": (1 << 32) + 1}, [0, 4]), ({"lens": ((1 << 32) + 1, 5)}, [0, 4]), ({"lens": (5, 6)}, [0, 4]), ({"max_len": 0}, [0, 4]),
             ({"max_len": 33}, [0, 4]), ({"sentinels": none}, [0, 4]), ({"sentinels": none, "final_sentinel": False}, [0, 4]),
             ({"sentinels": one}, [0, 4]), ({"flags": 4}, [0, 4]), ({"whole_word": True}, [0, 4]), ({}, [1, 4]), ({}, [0, 11]), ({}, [0, 5, 4])]
    for bad, starts in cases:
        with pytest.raises(_native.YabpeError) as e:
            ctx.span_corrupt(ids, None, np.asarray(starts, np.uint64), None, None, **{**ok, **bad})
        assert e.value.code == E_INVALID, (bad, starts)
        assert ctx.span_stats() == stats  # a refused call has changed nothing
    with pytest.raises(_native.YabpeError) as e:  # more than 2^36 ids: refused before anything is read or allocated
        ctx.span_corrupt(ids.ctypes.data, (1 << 36) + 1, None, None, None, **ok)
    assert e.value.code == E_CAPACITY and ctx.span_stats() == stats
    # no result came back: the C call leaves every output zero
    sp = _native.Span(0, 0, (1 << 32) + 1, (ctypes.c_uint64 * 31)(), 1, 1, ctypes.c_void_p(one.ctypes.data), 0, 0)
    outs = [ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_uint64(1), ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_uint64(1)]
    rc = _native.lib().yabpe_span_corrupt(ctx._h, ctypes.c_void_p(ids.ctypes.data), 10, None, 1, None, ctypes.byref(sp), *[ctypes.byref(o) for o in outs])
    assert rc == E_INVALID and not any(o.value for o in outs)
    assert len(ctx.span_corrupt_to_host(ids, None, [0, 4], None, None, **{**ok, "sentinels": one, "final_sentinel": False})[1]) == 3
    again = ctx.span_corrupt_to_host(ids, None, [0, 4], None, None, **ok)
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    for bad in ({"sentinels": []}, {"sentinels": sh.sentinels(1)}, {"sentinels": ["nope"]}, {"sentinels": "[MASK]"}, {"p": 1.5}, {"mean_span_length": 0.5},
                {"max_span_length": 33}, {"max_span_length": 0}, {"whole_word": True}, {"max_tokens": 0}, {"seed": -1}):
        with pytest.raises(ValueError):
            tok.corrupt_spans_array(ids, [0, 10], **{"sentinels": sh.sentinels(4), **bad})
    with pytest.raises(ValueError):
        tok.corrupt_spans_array(ids, [0, 4, 9], sentinels=sh.sentinels(4))  # doc_off must end at len(ids)
