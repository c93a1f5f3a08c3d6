"""GPU: BBPETokenizer.minhash_array (yabpe_minhash) against the plain-Python minhash_tokens, value for value: every n-gram
width and function count, each edge length of a piece as a single document (the last ones of several pieces: the atomicMin
path) and a batch of about 300 documents with those lengths between short ones; the band shapes; and encode_array_minhash
against encode_batch_minhash."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mask_helpers, minhash_helpers as mh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mask_helpers.tokenizer()


def check(tok, lens, num_perm, ngram, bands):
    exp_sig, exp_cnt, exp_keys = mh.contract(tuple(lens), num_perm, ngram, bands)
    ids, off = mh.flat(mh.documents(tuple(lens)))
    sig, cnt, keys = tok.minhash_array(ids, off, num_perm=num_perm, ngram=ngram, bands=bands, seed=7)
    assert (sig.dtype, cnt.dtype, sig.shape) == (np.uint32, np.uint64, (len(lens), num_perm))
    assert np.array_equal(cnt, exp_cnt) and np.array_equal(sig, exp_sig), (lens[:4], num_perm, ngram)
    assert keys is None if bands is None else (keys.dtype == np.uint64 and np.array_equal(keys, exp_keys))


@pytest.mark.parametrize("num_perm", mh.PERMS)
@pytest.mark.parametrize("ngram", mh.NGRAMS)
def test_signatures_match_plain_python(tok, ngram, num_perm):
    for n in mh.edge_lengths(ngram):
        check(tok, [n], num_perm, ngram, None)
    check(tok, mh.batch_lengths(ngram), num_perm, ngram, None)
    st = tok._device().minhash_stats()  # (of the batch: the two longest documents are of several pieces)
    assert st["n_multi_piece_docs"] == 2 and st["n_shingles"] == int(mh.contract(tuple(mh.batch_lengths(ngram)), num_perm, ngram, None)[1].sum())


@pytest.mark.parametrize("num_perm, bands", mh.BANDS)
def test_band_keys_match_plain_python(tok, num_perm, bands):
    check(tok, mh.batch_lengths(5), num_perm, 5, bands)


def test_encode_array_minhash_matches_encode_batch_minhash(tok):
    docs = mask_helpers.word_docs()[:60]
    kw = {"num_perm": 128, "ngram": 5, "bands": 32, "seed": 3}
    exp_sig, exp_cnt, exp_keys = tok.encode_batch_minhash(docs, **kw)
    sig, cnt, keys = tok.encode_array_minhash(docs, **kw)
    assert sig.tolist() == exp_sig and cnt.tolist() == exp_cnt and keys.tolist() == exp_keys
    sig, cnt, keys = tok.encode_array_minhash([], num_perm=64)
    assert sig.shape == (0, 64) and cnt.shape == (0,) and keys is None
