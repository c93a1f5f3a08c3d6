"""GPU: BBPETokenizer.encode_array_masked (yabpe_encode_words, yabpe_mask, then yabpe_layout_pad over the masked ids and over
the labels) against the plain-Python encode_batch_masked: max_length None, 8 and 1, BOS and EOS, both truncation and both
padding sides, whole-word masking on and off, no texts, and p = 0 against encode_array_padded."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu
BOS, EOS = 70001, 70002


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


@pytest.fixture(scope="module")
def docs():
    d = mh.word_docs()
    return d[:60]  # every special case of the shared set and some of the short documents


@pytest.mark.parametrize("max_length", [None, 8, 1])
def test_matches_plain_python(tok, docs, max_length):
    ran = 0
    for (bos, eos), trunc, side, whole_word in itertools.product(((None, None), (BOS, EOS), (BOS, None)), ("right", "left"), ("right", "left"),
                                                                 (False, True)):
        if max_length is not None and max_length < (bos is not None) + (eos is not None):
            continue
        kw = {"p": 0.4, "seed": 21, "first_doc": 3, "whole_word": whole_word, "bos_id": bos, "eos_id": eos, "truncation": trunc, "padding_side": side}
        exp_rows, exp_lab, exp_len = tok.encode_batch_masked(docs, max_length, **kw)
        rows, labels, lengths = tok.encode_array_masked(docs, max_length, **kw)
        assert (rows.dtype, labels.dtype, lengths.dtype) == (np.uint32, np.int32, np.uint32)
        assert rows.shape == labels.shape == (len(docs), len(exp_rows[0]))
        what = (max_length, bos, eos, trunc, side, whole_word)
        assert rows.tolist() == exp_rows and labels.tolist() == exp_lab and lengths.tolist() == exp_len, what
        # labels are -100 in BOS, EOS and pad slots: everywhere outside the content of the row
        L = rows.shape[1]
        for d in range(len(docs)):
            n = int(lengths[d])
            lo = L - n if side == "left" else 0
            content = range(lo + (bos is not None), lo + n - (eos is not None))
            assert all(labels[d, c] == mh.IGNORE for c in range(L) if c not in content), what
        ran += 1
    assert ran >= 8


def test_p_zero_is_the_padded_batch(tok, docs):
    for max_length, (bos, eos) in itertools.product((None, 8), ((None, None), (BOS, EOS))):
        rows, labels, lengths = tok.encode_array_masked(docs, max_length, p=0, bos_id=bos, eos_id=eos)
        plain_rows, plain_len = tok.encode_array_padded(docs, max_length, bos_id=bos, eos_id=eos)
        assert np.array_equal(rows, plain_rows) and np.array_equal(lengths, plain_len)
        assert np.all(labels == mh.IGNORE)


def test_the_mask_does_not_depend_on_the_cut(tok, docs):
    full_rows, full_lab, _ = tok.encode_array_masked(docs, None, p=0.5, seed=2)
    rows, lab, _ = tok.encode_array_masked(docs, 8, p=0.5, seed=2)
    w = min(8, full_rows.shape[1])
    keep = np.asarray([len(e[0]) for e in tok.encode_batch_with_words(docs)]) >= 8  # rows that are cut or full: no pad inside
    assert np.array_equal(rows[keep, :w], full_rows[keep, :w]) and np.array_equal(lab[keep, :w], full_lab[keep, :w]) and keep.any()


def test_no_texts_and_empty_texts(tok):
    for max_length in (None, 8):
        rows, labels, lengths = tok.encode_array_masked([], max_length)
        L = max_length or 0
        assert rows.shape == labels.shape == (0, L) and lengths.shape == (0,)
        assert (rows.dtype, labels.dtype, lengths.dtype) == (np.uint32, np.int32, np.uint32)
    rows, labels, lengths = tok.encode_array_masked(["", ""])
    assert rows.shape == labels.shape == (2, 0) and lengths.tolist() == [0, 0] and labels.dtype == np.int32
    rows, labels, lengths = tok.encode_array_masked(["", ""], 4, bos_id=BOS, p=1)
    pad = tok._vocab[b"[PAD]"]
    assert rows.tolist() == [[BOS, pad, pad, pad]] * 2 and np.all(labels == mh.IGNORE) and lengths.tolist() == [1, 1]
    with pytest.raises(ValueError):
        tok.encode_array_masked(["a"], mask_fraction=0.75, random_fraction=0.5)
