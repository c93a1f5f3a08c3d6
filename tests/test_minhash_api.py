"""CPU: the plain-Python MinHash contract (BBPETokenizer.minhash_params / minhash_tokens / minhash_jaccard) -- what the
kernels of csrc/yabpe_minhash_kernels.h are held to."""
from __future__ import annotations

import math

import pytest

from yet_another_bpe.synth import rnd_int
from yet_another_bpe.tokenizer import BBPETokenizer

TOK = BBPETokenizer()
M64 = (1 << 64) - 1


def test_params_are_a_pure_function_of_their_arguments():
    a, b = TOK.minhash_params(128, 3)
    assert (a, b) == TOK.minhash_params(128, 3) and (a, b) != TOK.minhash_params(128, 4)
    assert TOK.minhash_params(64, 3) == (a[:64], b[:64])  # function k does not depend on num_perm
    assert a == [rnd_int(3, 0x70, k) | 1 for k in range(128)] and b == [rnd_int(3, 0x71, k) for k in range(128)]


def test_signature_and_keys_restated_on_python_integers():
    ids, n, K = [0, 0xFFFFFFFF, 5, 5, 0, 7, 0xFFFFFFFF], 3, 6
    a, b = TOK.minhash_params(K, 9)
    hashes = []
    for w in range(len(ids) - n + 1):
        s = rnd_int(0, 0x68, n)
        for t in ids[w:w + n]:
            s = rnd_int(s, 0, t)  # = mix(s + G * (t + 1))
        hashes.append(s >> 32)
    sig = [min(((a[k] * h + b[k]) & M64) >> 32 for h in hashes) for k in range(K)]
    keys = []
    for band in range(3):
        s = rnd_int(0, 0x6B, band)
        for v in sig[2 * band:2 * band + 2]:
            s = rnd_int(s, 0, v)
        keys.append(s)
    short = rnd_int(rnd_int(rnd_int(0, 0x68, 2), 0, 4), 0, 0)  # a document shorter than n: one shingle of all its ids
    got_sig, got_cnt, got_keys = TOK.minhash_tokens([ids, [], [4, 0]], num_perm=K, ngram=n, bands=3, seed=9)
    assert got_sig == [sig, [0xFFFFFFFF] * K, [((a[k] * (short >> 32) + b[k]) & M64) >> 32 for k in range(K)]]
    assert got_cnt == [5, 0, 1] and got_keys[0] == keys


@pytest.mark.parametrize("n, doc_a, doc_b", [(1, [1, 2, 3], [3, 2, 1, 1, 2]), (2, [1, 2, 1, 2, 1], [2, 1, 2]), (5, [4, 9], [4, 9])])
def test_equal_shingle_sets_give_equal_signatures(n, doc_a, doc_b):
    sig, cnt, keys = TOK.minhash_tokens([doc_a, doc_b], ngram=n, bands=16, seed=1)
    assert sig[0] == sig[1] and keys[0] == keys[1] and TOK.minhash_jaccard(sig[0], sig[1]) == 1.0
    assert cnt == [max(1, len(doc_a) - n + 1), max(1, len(doc_b) - n + 1)]


@pytest.mark.parametrize("shared, each", [(400, 200), (800, 100), (100, 450)])
def test_planted_pair_estimates_its_jaccard_index(shared, each):
    """Two documents of distinct ids, ngram = 1: J = shared / (shared + 2 each); five binomial standard errors at num_perm = 512."""
    doc_a, doc_b = list(range(shared + each)), list(range(each, shared + 2 * each))
    J = shared / (shared + 2 * each)
    sig, _cnt, _keys = TOK.minhash_tokens([doc_a, doc_b], num_perm=512, ngram=1, seed=0)
    est = TOK.minhash_jaccard(sig[0], sig[1])
    print(J, est)
    assert abs(est - J) <= 5 * math.sqrt(J * (1 - J) / 512)


@pytest.mark.parametrize("bad", [{"num_perm": 128, "bands": 5}, {"ngram": 0}, {"ngram": 33}, {"num_perm": 0}, {"num_perm": 1025}, {"seed": -1}])
def test_arguments_out_of_range_are_refused(bad):
    for call in (lambda: TOK.minhash_tokens([[1, 2, 3]], **bad), lambda: TOK.encode_batch_minhash(["a"], **bad),
                 lambda: TOK.minhash_array([1, 2, 3], [0, 3], **bad)):  # (refused before a device is looked for)
        with pytest.raises(ValueError):
            call()
