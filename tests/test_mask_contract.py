"""CPU: BBPETokenizer.mask_tokens and encode_batch_masked, the plain-Python contract of yabpe_mask: a seeded 80/10/10 masking
draw that is a pure function of (seed, document index, unit), never touches a special and, with whole_word, treats all
tokens of a word alike."""
from __future__ import annotations

import math

import numpy as np
import pytest

from tests import mask_helpers as mh

MASK_ID, N_RANDOM = 5000, 1000
LENS = [0, 5, 300, 1, 0, 41, 700, 3]


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


@pytest.fixture(scope="module")
def batch():
    """ids in [2000, 3000): neither MASK_ID nor below N_RANDOM, so mh.kinds reads every token's kind exactly"""
    ids, words, special = mh.synth_batch(LENS)
    return [[i + 2000 for i in doc] for doc in ids], words, special


def run(tok, batch, use_special=True, **kw):
    ids, words, special = batch
    kw = {"mask_id": MASK_ID, "n_random": N_RANDOM, **kw}
    inputs, labels = tok.mask_tokens(ids, words, special if use_special else None, **kw)
    assert [len(r) for r in inputs] == [len(r) for r in labels] == [len(r) for r in ids]
    return inputs, labels, mh.kinds(ids, inputs, labels, special if use_special else None, MASK_ID)


def test_p_zero_and_one(tok, batch):
    ids, _words, special = batch
    inputs, labels, _k = run(tok, batch, p=0)
    assert inputs == ids and all(x == mh.IGNORE for row in labels for x in row)
    for whole_word in (False, True):
        inputs, labels, kinds = run(tok, batch, p=1, whole_word=whole_word)
        for d in range(len(ids)):
            for j, sp in enumerate(special[d]):
                assert (kinds[d][j] == "protected") == sp
                if sp:
                    assert inputs[d][j] == ids[d][j] and labels[d][j] == mh.IGNORE
                else:
                    assert labels[d][j] == ids[d][j]
    inputs, labels, kinds = run(tok, batch, use_special=False, p=1)  # without special_batch nothing is protected
    assert labels == ids


@pytest.mark.parametrize("fractions, kind", [((1, 0), "masked"), ((0, 1), "random"), ((0, 0), "kept")])
def test_fractions(tok, batch, fractions, kind):
    ids, _words, _special = batch
    inputs, labels, kinds = run(tok, batch, p=0.5, mask_fraction=fractions[0], random_fraction=fractions[1])
    got = {k for row in kinds for k in row}
    assert got == {"protected", "unselected", kind}
    for d, row in enumerate(kinds):
        for j, k in enumerate(row):
            if k == "masked":
                assert inputs[d][j] == MASK_ID
            elif k == "random":
                assert 0 <= inputs[d][j] < N_RANDOM
            else:
                assert inputs[d][j] == ids[d][j]


def test_a_label_is_the_original_id_or_ignore(tok, batch):
    ids, _words, _special = batch
    for whole_word in (False, True):
        inputs, labels, kinds = run(tok, batch, p=0.3, whole_word=whole_word)
        for d in range(len(ids)):
            for j in range(len(ids[d])):
                assert labels[d][j] in (ids[d][j], mh.IGNORE)
                if labels[d][j] == mh.IGNORE:
                    assert inputs[d][j] == ids[d][j]


def test_whole_word_shares_selection_and_kind(tok, batch):
    ids, words, special = batch
    inputs, labels, kinds = run(tok, batch, p=0.4, whole_word=True, seed=3)
    multi = 0
    for d in range(len(ids)):
        by_word = {}
        for j, w in enumerate(words[d]):
            if not special[d][j]:
                by_word.setdefault(w, []).append(kinds[d][j])
        for w, ks in by_word.items():
            assert len(set(ks)) == 1, (d, w, ks)
            multi += len(ks) > 1 and ks[0] != "unselected"
    assert multi > 20  # (the batch has words of several tokens that were selected)
    # ... and the random replacement is drawn per token: the tokens of a randomised word do not all get one id
    inputs, _labels, kinds = run(tok, batch, p=1, whole_word=True, mask_fraction=0, random_fraction=1)
    d = 6
    groups = {}
    for j, w in enumerate(words[d]):
        if kinds[d][j] == "random":
            groups.setdefault(w, set()).add(inputs[d][j])
    assert any(len(g) > 1 for g in groups.values())
    # without whole_word the tokens of a word are drawn one by one
    _i, _l, kinds = run(tok, batch, p=0.4, seed=3)
    assert any(len({kinds[6][j] for j, w in enumerate(words[6]) if w == x and not special[6][j]}) > 1 for x in set(words[6]))


def test_a_document_depends_on_seed_and_index_alone(tok):
    (a, b), (wa, wb), (sa, sb) = mh.synth_batch([60, 90], seed=4)
    for whole_word in (False, True):
        kw = {"mask_id": MASK_ID, "n_random": N_RANDOM, "p": 0.5, "seed": 11, "whole_word": whole_word}
        both = tok.mask_tokens([a, b], [wa, wb], [sa, sb], first_doc=5, **kw)
        alone = tok.mask_tokens([b], [wb], [sb], first_doc=6, **kw)
        assert (both[0][1], both[1][1]) == (alone[0][0], alone[1][0])
        shifted = tok.mask_tokens([b], [wb], [sb], first_doc=7, **kw)
        assert shifted != alone
        huge = tok.mask_tokens([a, b], [wa, wb], [sa, sb], first_doc=(1 << 64) - 1, **kw)  # first_doc + d wraps at 2^64
        assert huge[0][1] == tok.mask_tokens([b], [wb], [sb], first_doc=0, **kw)[0][0]


def test_seeds_differ(tok, batch):
    assert run(tok, batch, seed=1)[0] != run(tok, batch, seed=2)[0]
    assert run(tok, batch, seed=1)[:2] == run(tok, batch, seed=1)[:2]


def five_sigma(n, q):
    return 5 * math.sqrt(n * q * (1 - q))


@pytest.mark.parametrize("whole_word", [False, True])
def test_rates(tok, whole_word):
    """Over n >= 20,000 unprotected units the selected count lies within 5 sqrt(n p (1 - p)) of n p, and among the s selected
    each kind within 5 sqrt(s q (1 - q)) of s q for q = 0.8 / 0.1 / 0.1.  Fixed seeds.  (Whole-word mode: one token a word,
    so that the units are independent draws.)"""
    lens = [700] * 20 + [37] * 300
    ids, _words, special = mh.synth_batch(lens, seed=6)
    ids = [[i + 2000 for i in doc] for doc in ids]
    words = [list(range(0, 2 * len(doc), 2)) for doc in ids]
    inputs, labels = tok.mask_tokens(ids, words, special, mask_id=MASK_ID, n_random=N_RANDOM, p=0.15, seed=2024, whole_word=whole_word)
    count = {}
    for row in mh.kinds(ids, inputs, labels, special, MASK_ID):
        for k in row:
            count[k] = count.get(k, 0) + 1
    n = sum(v for k, v in count.items() if k != "protected")
    assert n >= 20000 and count["protected"] == sum(sum(s) for s in special)
    selected = n - count["unselected"]
    assert abs(selected - n * 0.15) <= five_sigma(n, 0.15), (selected, n)
    for kind, q in (("masked", 0.8), ("random", 0.1), ("kept", 0.1)):
        assert abs(count[kind] - selected * q) <= five_sigma(selected, q), (kind, count[kind], selected)


def test_defaults(tok):
    ids = [[1, 2, 3, 4] * 50]
    inputs, labels = tok.mask_tokens(ids, p=1, mask_fraction=1, random_fraction=0)
    assert set(inputs[0]) == {tok._vocab[b"[MASK]"]} and labels == ids
    inputs, _labels = tok.mask_tokens(ids, p=1, mask_fraction=0, random_fraction=1)
    top = max(tok._vocab.values())
    assert max(inputs[0]) <= top and len(set(inputs[0])) > 50
    assert tok.mask_tokens([]) == ([], [])
    assert tok.mask_tokens(np.asarray([[7, 8]], dtype=np.uint32), p=0) == ([[7, 8]], [[mh.IGNORE, mh.IGNORE]])


def test_value_errors(tok):
    ids = [[1, 2, 3]]
    from yet_another_bpe.tokenizer import BBPETokenizer

    with pytest.raises(ValueError, match="MASK"):
        BBPETokenizer(vocab={b"a": 0}).mask_tokens(ids)
    with pytest.raises(ValueError, match="whole_word"):
        tok.mask_tokens(ids, whole_word=True)
    with pytest.raises(ValueError, match="at most 1"):
        tok.mask_tokens(ids, mask_fraction=0.75, random_fraction=0.5)
    for name in ("p", "mask_fraction", "random_fraction"):
        for bad in (-0.1, 1.5, float("nan"), "x", None):
            with pytest.raises(ValueError):
                tok.mask_tokens(ids, **{name: bad})
    for name in ("seed", "first_doc"):
        for bad in (-1, 1 << 64, 1.5, "x"):
            with pytest.raises(ValueError, match=name):
                tok.mask_tokens(ids, **{name: bad})
    for bad in (-1, 1 << 32, 1.5):
        with pytest.raises(ValueError):
            tok.mask_tokens(ids, mask_id=bad)
        with pytest.raises(ValueError, match="n_random"):
            tok.mask_tokens(ids, n_random=bad)
    with pytest.raises(ValueError, match="n_random"):
        tok.mask_tokens(ids, n_random=0)
    assert tok.mask_tokens(ids, n_random=0, random_fraction=0, p=0)[0] == ids  # (n_random is not needed without random draws)
    with pytest.raises(ValueError):
        tok.encode_batch_masked(["a"], mask_fraction=0.75, random_fraction=0.5)
    with pytest.raises(ValueError):
        tok.encode_batch_masked(["a"], max_length=1, bos_id=1, eos_id=2)


@pytest.mark.parametrize("max_length", [None, 8, 1])
def test_encode_batch_masked(tok, max_length):
    docs = mh.word_docs()[:40]
    pad = tok._vocab[b"[PAD]"]
    for bos, eos, trunc, side, whole_word in ((None, None, "right", "right", False), (70001, 70002, "left", "left", True),
                                              (70001, None, "right", "left", True)):
        if max_length is not None and max_length < (bos is not None) + (eos is not None):
            continue
        kw = {"bos_id": bos, "eos_id": eos, "truncation": trunc, "padding_side": side}
        rows, labels, lengths = tok.encode_batch_masked(docs, max_length, p=0.5, seed=8, whole_word=whole_word, **kw)
        plain_rows, plain_len = tok.encode_batch_padded(docs, max_length, **kw)
        assert lengths == plain_len and [len(r) for r in rows] == [len(r) for r in plain_rows] == [len(r) for r in labels]
        # the mask is drawn before the cut: every kept slot holds what mask_tokens gives that token of the whole document
        enc = tok.encode_batch_with_words(docs)
        inputs, labs = tok.mask_tokens([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], p=0.5, seed=8, whole_word=whole_word)
        changed = 0
        for d in range(len(docs)):
            L, n, added = len(rows[d]), len(enc[d][0]), (bos is not None) + (eos is not None)
            keep = min(n, L - added)
            src = list(range(keep)) if trunc == "right" else list(range(n - keep, n))
            seq = ([bos] if bos is not None else []) + [inputs[d][j] for j in src] + ([eos] if eos is not None else [])
            lab = ([mh.IGNORE] if bos is not None else []) + [labs[d][j] for j in src] + ([mh.IGNORE] if eos is not None else [])
            fill = L - len(seq)
            assert rows[d] == (seq + [pad] * fill if side == "right" else [pad] * fill + seq)
            assert labels[d] == (lab + [mh.IGNORE] * fill if side == "right" else [mh.IGNORE] * fill + lab)
            changed += rows[d] != plain_rows[d]
        assert changed or max_length == 1
    rows, labels, lengths = tok.encode_batch_masked(docs, max_length, p=0)
    assert (rows, lengths) == tok.encode_batch_padded(docs, max_length) and all(x == mh.IGNORE for r in labels for x in r)
    assert tok.encode_batch_masked([], max_length) == ([], [], [])
