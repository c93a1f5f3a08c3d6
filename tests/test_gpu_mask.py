"""GPU: BBPETokenizer.mask_array (yabpe_mask) bit for bit against the plain-Python mask_tokens on the document sets of the CPU
model test (empty documents, hundreds of documents in a block, a document over several blocks, no ids, no doc_off), inputs
as host arrays and as the device results of yabpe_encode_words, the call's statistics, results that outlive later encode and
layout calls, and every refused argument."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from tests import mask_helpers as mh
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
MASK_ID, N_RANDOM = 5000, 777
E_INVALID = -1
T = BBPETokenizer._dropout_threshold


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


def flat_i(batch):
    return [x for r in batch for x in r]


@pytest.mark.parametrize("name, lens, with_off", mh.LENGTH_SETS, ids=[s[0] for s in mh.LENGTH_SETS])
def test_matches_plain_python(tok, name, lens, with_off):
    ids_b, words_b, special_b = mh.synth_batch(lens)
    ids, words, special = mh.flat(ids_b, np.uint32), mh.flat(words_b, np.uint32), mh.flat(special_b, bool)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    ctx = tok._device()
    for p, whole_word, seed, first_doc in itertools.product((0, 0.15, 0.5, 1), (False, True), (0, 12345), (0, 1 << 40)):
        kw = {"mask_id": MASK_ID, "n_random": N_RANDOM, "p": p, "seed": seed, "whole_word": whole_word, "first_doc": first_doc}
        what = (name, p, whole_word, seed, first_doc)
        exp_in, exp_lab = tok.mask_tokens(ids_b, words_b, special_b, **kw)
        if with_off:
            got_in, got_lab = tok.mask_array(ids, off, words, special, **kw)
        else:  # one document, doc_off NULL: through the binding
            got_in, got_lab = ctx.mask_to_host(ids, None, None, None, mh.packed_words(words_b, special_b), seed=seed, first_doc=first_doc,
                                               select=T(p), mask=T(0.8), random=T(0.1), mask_id=MASK_ID, n_random=N_RANDOM, whole_word=whole_word)
        assert got_in.dtype == np.uint32 and got_lab.dtype == np.int32
        assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab), what
        # the statistics of the call against the Python result (the ids are below 1000: MASK_ID appears only by masking)
        st = ctx.mask_stats()
        kinds = mh.kinds(ids_b, exp_in, exp_lab, special_b, MASK_ID)
        n_sel = sum(x != mh.IGNORE for x in flat_i(exp_lab))
        assert (st["n_ids"], st["n_docs"]) == (len(ids), len(lens)), what
        assert st["n_protected"] == sum(k == "protected" for k in flat_i(kinds)) == int(special.sum()), what
        assert st["n_selected"] == n_sel == st["n_masked"] + st["n_random"] + st["n_kept"], what
        assert st["n_masked"] == sum(x == MASK_ID for x in flat_i(exp_in)), what
        if not whole_word and with_off:  # without words and specials: nothing is protected
            exp_in, exp_lab = tok.mask_tokens(ids_b, **{**kw, "whole_word": False})
            got_in, got_lab = tok.mask_array(ids, off, **{**kw, "whole_word": False})
            assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab), what
            assert ctx.mask_stats()["n_protected"] == 0
            exp_in, exp_lab = tok.mask_tokens(ids_b, None, special_b, **kw)  # specials alone
            got_in, got_lab = tok.mask_array(ids, off, None, special, **kw)
            assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab), what


def test_fractions(tok):
    lens = [3, 0, 400, 1, 1, 90]
    ids_b, words_b, special_b = mh.synth_batch(lens, seed=3)
    ids, words, special = mh.flat(ids_b, np.uint32), mh.flat(words_b, np.uint32), mh.flat(special_b, bool)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    for fm, fr in ((1, 0), (0, 1), (0, 0), (0.5, 0.5), (0.8, 0.1)):
        kw = {"mask_id": MASK_ID, "n_random": N_RANDOM, "p": 0.6, "seed": 9, "whole_word": True, "mask_fraction": fm, "random_fraction": fr}
        exp_in, exp_lab = tok.mask_tokens(ids_b, words_b, special_b, **kw)
        got_in, got_lab = tok.mask_array(ids, off, words, special, **kw)
        assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab), (fm, fr)
    got_in, _ = tok.mask_array(ids, off, p=1, mask_fraction=1, random_fraction=0)  # the defaults: [MASK] of the vocab
    assert set(got_in.tolist()) == {tok._vocab[b"[MASK]"]}


def test_device_results_of_encode_words_go_straight_in(tok):
    docs = mh.word_docs()
    enc = tok.encode_batch_with_words(docs)
    ctx = tok._device()
    data, starts = tok._device_input(docs)
    for whole_word in (False, True):
        di, dd, dw, ni = ctx.encode_words(data, doc_starts=starts)
        before = [ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dw, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)]
        got_in, got_lab = ctx.mask_to_host(di, ni, dd, len(docs), dw, seed=4, first_doc=2, select=T(0.3), mask=T(0.8), random=T(0.1),
                                           mask_id=MASK_ID, n_random=N_RANDOM, whole_word=whole_word)
        exp_in, exp_lab = tok.mask_tokens([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], mask_id=MASK_ID, n_random=N_RANDOM,
                                          p=0.3, seed=4, first_doc=2, whole_word=whole_word)
        assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab)
        assert ctx.mask_stats()["n_protected"] == sum(sum(e[2]) for e in enc) > 0
        after = [ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dw, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))  # the inputs are left alone
    # whole-word masking of real text (the last round above): the tokens of a word go together
    kinds = mh.kinds([e[0] for e in enc], exp_in, exp_lab, [e[2] for e in enc], MASK_ID)
    for d, e in enumerate(enc):
        by_word = {}
        for j, w in enumerate(e[1]):
            by_word.setdefault(w, set()).add(kinds[d][j] == "unselected")
        assert all(len(v) == 1 for v in by_word.values())


def test_results_outlive_later_encode_and_layout_calls(tok):
    lens = [5, 0, 300, 2]
    ids_b, words_b, special_b = mh.synth_batch(lens, seed=5)
    ids, packed = mh.flat(ids_b, np.uint32), mh.packed_words(words_b, special_b)
    ctx = tok._device()
    kw = {"seed": 1, "select": T(0.5), "mask": T(0.8), "random": T(0.1), "mask_id": MASK_ID, "n_random": N_RANDOM}
    mi, ml = ctx.mask(ids, None, mh.starts(lens), None, packed, **kw)
    first = (ctx.d2h(mi, 4 * len(ids), np.uint32), ctx.d2h(ml, 4 * len(ids), np.uint32))
    tok.encode_array(mh.word_docs()[:20])
    tok.encode_array_padded(mh.word_docs()[:20], 16)
    again = (ctx.d2h(mi, 4 * len(ids), np.uint32), ctx.d2h(ml, 4 * len(ids), np.uint32))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    exp_in, exp_lab = tok.mask_tokens(ids_b, words_b, special_b, mask_id=MASK_ID, n_random=N_RANDOM, p=0.5, seed=1)
    assert first[0].tolist() == flat_i(exp_in) and first[1].view(np.int32).tolist() == flat_i(exp_lab)
    got_in, got_lab = ctx.mask_to_host(ids, None, mh.starts(lens), None, packed, **{**kw, "seed": 2})  # a new call still works
    exp_in, exp_lab = tok.mask_tokens(ids_b, words_b, special_b, mask_id=MASK_ID, n_random=N_RANDOM, p=0.5, seed=2)
    assert got_in.tolist() == flat_i(exp_in) and got_lab.tolist() == flat_i(exp_lab)
    ctx.mask_free()
    ctx.mask_free()


def test_refused_arguments(tok):
    from yet_another_bpe import _native

    ids = np.arange(10, dtype=np.uint32)
    ctx = tok._device()
    ok = {"select": T(0.5), "mask": T(0.8), "random": T(0.1), "mask_id": MASK_ID, "n_random": N_RANDOM}
    good = ctx.mask_to_host(ids, None, [0, 4], None, None, **ok)
    stats = ctx.mask_stats()
    cases = [({"select": (1 << 32) + 1}, [0, 4], None), ({"mask": (1 << 32) + 1}, [0, 4], None), ({"random": (1 << 32) + 1}, [0, 4], None),
             ({"mask": T(0.75), "random": T(0.5)}, [0, 4], None), ({"n_random": 0}, [0, 4], None), ({"flags": 2}, [0, 4], None),
             ({"whole_word": True}, [0, 4], None), ({}, [1, 4], None), ({}, [0, 11], None), ({}, [0, 5, 4], None)]
    for bad, starts, words in cases:
        with pytest.raises(_native.YabpeError) as e:
            ctx.mask(ids, None, np.asarray(starts, np.uint64), None, words, **{**ok, **bad})
        assert e.value.code == E_INVALID, (bad, starts)
        assert ctx.mask_stats() == stats  # a refused call has changed nothing
    # no result came back: the C call leaves both pointers NULL
    import ctypes

    m = _native.Mask(0, 0, (1 << 32) + 1, 0, 0, 0, 1, _native.MASK_IGNORE, 0)
    di, dl = ctypes.c_void_p(1), ctypes.c_void_p(1)
    rc = _native.lib().yabpe_mask(ctx._h, ctypes.c_void_p(ids.ctypes.data), 10, None, 1, None, ctypes.byref(m), ctypes.byref(di), ctypes.byref(dl))
    assert rc == E_INVALID and not di.value and not dl.value
    assert ctx.mask_to_host(ids, None, [0, 4], None, None, **{**ok, "random": 0, "n_random": 0})[0].shape == (10,)  # (no random draws: n_random unused)
    again = ctx.mask_to_host(ids, None, [0, 4], None, None, **ok)
    assert np.array_equal(good[0], again[0]) and np.array_equal(good[1], again[1])
    with pytest.raises(ValueError):
        tok.mask_array(ids, [0, 4, 9])  # doc_off must end at len(ids)
    with pytest.raises(ValueError):
        tok.mask_array(ids, [0, 10], whole_word=True)
