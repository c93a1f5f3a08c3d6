"""CPU: the plain-Python clustering rule (BBPETokenizer.minhash_clusters / encode_batch_clusters) -- what the kernels of
csrc/yabpe_cluster_kernels.h are held to."""
from __future__ import annotations

import numpy as np
import pytest

from tests import mask_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

TOK = BBPETokenizer()


def labels(n, pairs):
    """Connected components of explicit pairs, every document labelled with its component's minimum."""
    lab = list(range(n))
    changed = True
    while changed:
        changed = False
        for a, b in pairs:
            if lab[a] != lab[b]:
                lab[a] = lab[b] = min(lab[a], lab[b])
                changed = True
    return lab


@pytest.mark.parametrize("seed", range(6))
def test_star_to_anchor_has_the_components_of_all_pairs_in_a_bucket(seed):
    rng = np.random.default_rng(seed)
    n, B = 40, 3
    keys = rng.integers(0, 12, (n, B)).astype(np.uint64)  # few values: large buckets, the same value in several bands
    cnt = rng.integers(0, 4, n).astype(np.uint64)
    pairs = [(a, b) for a in range(n) for b in range(a) if cnt[a] and cnt[b] and (keys[a] == keys[b]).any()]
    cluster, st = TOK.minhash_clusters(None, keys, cnt)
    assert cluster == labels(n, pairs)
    assert st["n_participating"] == int((cnt > 0).sum()) and st["n_entries"] == B * st["n_participating"]
    assert st["n_accepted"] == st["n_candidates"] and st["n_clusters"] == len(set(cluster)) and st["n_docs"] == n


def test_hand_cases():
    u = lambda rows: np.asarray(rows, np.uint64)
    # a chain: d2 ~ d1 in band 1, d1 ~ d0 in band 0 -> one cluster labelled 0; d3 alone
    assert TOK.minhash_clusters(None, u([[1, 2], [1, 3], [4, 3], [5, 6]]))[0] == [0, 0, 0, 3]
    # an equal value in two different bands does not join
    assert TOK.minhash_clusters(None, u([[7, 1], [2, 7]]))[0] == [0, 1]
    # documents without shingles stay alone among identical rows
    cluster, st = TOK.minhash_clusters(None, u([[9, 9]] * 5), [0, 1, 0, 1, 1])
    assert cluster == [0, 1, 2, 1, 1] and (st["n_participating"], st["n_entries"], st["n_clusters"]) == (3, 6, 3)
    # a pair that both bands give is one candidate
    assert TOK.minhash_clusters(None, u([[1, 2], [1, 2], [1, 5]]))[1]["n_candidates"] == 2
    # the min_agree boundary: rows agree in 3 of 4 slots
    sig = [[1, 2, 3, 4], [1, 2, 3, 9]]
    accepted, st3 = TOK.minhash_clusters(sig, u([[1], [1]]), min_agree=3)
    rejected, st4 = TOK.minhash_clusters(sig, u([[1], [1]]), min_agree=4)
    assert (accepted, st3["n_accepted"], rejected, st4["n_accepted"], st4["n_candidates"]) == ([0, 0], 1, [0, 1], 0, 1)


@pytest.mark.parametrize("sig, keys, cnt, m", [
    (None, np.zeros((2, 0), np.uint64), None, 0), (None, np.zeros((2, 1025), np.uint64), None, 0), (None, np.zeros(4, np.uint64), None, 0),
    (np.zeros((2, 0), np.uint32), [[1], [1]], None, 0), (np.zeros((2, 1025), np.uint32), [[1], [1]], None, 0),
    (np.zeros((3, 4), np.uint32), [[1], [1]], None, 0), (np.zeros((2, 4), np.uint32), [[1], [1]], None, 5),
    (np.zeros((2, 4), np.uint32), [[1], [1]], None, -1), (None, [[1], [1]], None, 1), (None, [[1], [1]], [1, 1, 1], 0),
    (None, [[1], [1]], None, 0.5)])
def test_arguments_out_of_range_are_refused(sig, keys, cnt, m):
    for call in (TOK.minhash_clusters, TOK.minhash_clusters_array):  # (refused before a device is looked for)
        with pytest.raises(ValueError):
            call(sig, keys, cnt, min_agree=m)


@pytest.mark.parametrize("bad", [{}, {"bands": 5}, {"bands": 32, "min_agree": 129}, {"bands": 32, "min_agree": -1}, {"bands": 32, "ngram": 0}])
def test_batch_arguments_are_refused_before_any_work(bad):
    for call in (TOK.encode_batch_clusters, TOK.encode_array_clusters):
        with pytest.raises(ValueError):
            call(["a"], **bad)


def test_one_word_edits_land_in_the_originals_cluster():
    tok = mask_helpers.tokenizer()
    words = "the quick brown fox jumps over a lazy dog while seven other animals watch from behind some old trees near our quiet river".split()
    rng = np.random.default_rng(0)
    originals = [" ".join(rng.permutation(words).tolist() * 3) for _ in range(6)]
    copies = [o.replace(" ", " very ", 1) for o in originals[:3]] + [originals[1] + " again"]
    cluster, cnt = tok.encode_batch_clusters(originals + copies + [""], num_perm=128, ngram=3, bands=32, seed=1, min_agree=64)
    assert cluster == [0, 1, 2, 3, 4, 5, 0, 1, 2, 1, 10] and cnt[10] == 0 and len(cnt) == 11
