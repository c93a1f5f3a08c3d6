"""GPU: BBPETokenizer.minhash_clusters_array (yabpe_minhash_cluster) against the plain-Python minhash_clusters -- the labels and
every integer statistic, exactly: each (num_perm, bands) shape over the hand-built corpora of cluster_helpers.py at three
min_agree values; a table forced to a load near 1; 0 and 1 documents; yabpe_minhash's device results passed straight in;
encode_array_clusters against encode_batch_clusters; each error code."""
from __future__ import annotations

import numpy as np
import pytest

from tests import cluster_helpers as ch, mask_helpers
from yet_another_bpe import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok():
    return mask_helpers.tokenizer()


def check(tok, sig, keys, cnt, m):
    exp, exp_st = tok.minhash_clusters(sig, keys, cnt, min_agree=m)
    got, st = tok.minhash_clusters_array(sig, keys, cnt, min_agree=m)
    print(m, exp_st, {k: st[k] for k in exp_st}, st["n_slots"])
    assert got.dtype == np.uint32 and got.tolist() == exp
    assert {k: st[k] for k in exp_st} == exp_st
    return st


@pytest.mark.parametrize("K, B", ch.SHAPES)
@pytest.mark.parametrize("name", ch.CORPORA)
def test_clusters_match_plain_python(tok, name, K, B):
    sig, keys, cnt = ch.corpus(name, K, B)
    for m in (0, ch.mid(K), K):
        st = check(tok, sig, keys, cnt, m)
    assert st["n_slots"] == max(1 << 10, 1 << (2 * len(keys) * B - 1).bit_length())


def test_table_at_a_load_near_one(tok):
    """250 documents x 4 bands in a table forced to 2^10 slots: long chains that wrap around the table's end."""
    sig, keys, cnt = ch.corpus("cross_band", 64, 4, n=250)
    keys[200:240, 1] = keys[200, 1]
    ctx = tok._device()
    ctx.set_option("cluster_slots_log2", 10)
    try:
        assert check(tok, sig, keys, None, ch.mid(64))["n_slots"] == 1 << 10
        ctx.set_option("cluster_slots_log2", 9)  # fewer than entries + 1
        with pytest.raises(_native.YabpeError) as e:
            tok.minhash_clusters_array(sig, keys)
        assert e.value.code == _native.E_INVALID
    finally:
        ctx.set_option("cluster_slots_log2", 0)


def test_no_document_and_one_document(tok):
    for n in (0, 1):
        got, st = tok.minhash_clusters_array(np.zeros((n, 8), np.uint32), np.zeros((n, 2), np.uint64), None, min_agree=8)
        assert got.tolist() == list(range(n)) and (st["n_docs"], st["n_clusters"], st["n_candidates"]) == (n, n, 0)


def test_minhash_device_results_go_straight_in_and_stay(tok):
    docs = mask_helpers.word_docs()[:60]
    docs += docs[8:20]  # (repeats: each joins its original)
    kw = {"num_perm": 128, "ngram": 5, "bands": 32, "seed": 3}
    exp, exp_cnt = tok.encode_batch_clusters(docs, min_agree=100, **kw)
    got, cnt = tok.encode_array_clusters(docs, min_agree=100, **kw)
    assert got.tolist() == exp and cnt.tolist() == exp_cnt and len(set(exp)) < len(exp)
    sig, cnt, keys = tok.encode_array_minhash(docs, **kw)  # (the buffers of this call: the context's last yabpe_minhash)
    ctx = tok._device()
    ids, off = tok.encode_array(docs)
    ds, dn, dk, nd = ctx.minhash(ids, None, off[:-1].astype(np.uint64), None, **kw)
    assert ctx.minhash_cluster_to_host(ds, dk, dn, nd, num_perm=128, bands=32, min_agree=100).tolist() == exp
    assert np.array_equal(ctx.d2h(ds, sig.nbytes, np.uint32), sig.ravel()) and np.array_equal(ctx.d2h(dk, keys.nbytes, np.uint64), keys.ravel())
    assert np.array_equal(ctx.d2h(dn, cnt.nbytes, np.uint64), cnt)
    assert tok.encode_array_clusters([], bands=4)[0].shape == (0,)


@pytest.mark.parametrize("code, sig, keys, kw", [
    (_native.E_INVALID, None, [[1]], {"num_perm": 4, "bands": 0}), (_native.E_INVALID, None, [[1]], {"num_perm": 0, "bands": 1}),
    (_native.E_INVALID, None, [[1]], {"num_perm": 1025, "bands": 1}), (_native.E_INVALID, None, [[1]], {"num_perm": 4, "bands": 1025}),
    (_native.E_INVALID, [[1, 2]], [[1]], {"num_perm": 2, "bands": 1, "min_agree": 3}),
    (_native.E_INVALID, None, [[1]], {"num_perm": 2, "bands": 1, "min_agree": 1}), (_native.E_INVALID, None, None, {"num_perm": 2, "bands": 1}),
    (_native.E_CAPACITY, None, [[1]], {"num_perm": 2, "bands": 1024, "n_docs": (1 << 20) + 1})])
def test_error_codes(tok, code, sig, keys, kw):
    """(the capacity case is refused before anything is read: its one row of keys stands for 2^20 + 1)"""
    with pytest.raises(_native.YabpeError) as e:
        tok._device().minhash_cluster(sig, keys, None, kw.pop("n_docs", 1), **kw)
    assert e.value.code == code
