"""CPU: the contract of the plain-Python fill-in-the-middle calls -- BBPETokenizer.fim_tokens, fim_cuts and encode_batch_fim:
the document back from the pieces of a sequence, at token and at character level; a slice of a batch under a shifted
first_doc; the labels of both loss modes; the refused arguments; and the statistical contract on 20,000 documents.

The statistical bound is derived, not measured: every document draws its mode from r = rnd(Kd, 0x61, 0) with a key of its
own, so the indicators "transformed" are independent Bernoulli(q) variables, q = Tf / 2^32, and their count over n documents
has the standard deviation sqrt(n q (1 - q)); the same holds for "SPM" among the transformed documents with q = Ts / 2^32 and
n the number of transformed documents.  The test allows five standard deviations and nothing more."""
from __future__ import annotations

import math

import pytest

from tests import fim_helpers as fh
from tests import mask_helpers as mh

SENT = {"pre": fh.PRE, "suf": fh.SUF, "mid": fh.MID}


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


def split(seq, info, eot):
    """a sequence and its info -> (P, M, S), the sentinels checked on the way"""
    mode, p, m, s = info
    if mode == 0:
        assert len(seq) == p + m + s
        return seq[:p], seq[p:p + m], seq[p + m:]
    assert len(seq) == 3 + p + m + s + (eot is not None)
    if eot is not None:
        assert seq[-1] == eot
    if mode == 1:
        assert (seq[0], seq[1 + p], seq[2 + p + s]) == (fh.PRE, fh.SUF, fh.MID)
        return seq[1:1 + p], seq[3 + p + s:3 + p + s + m], seq[2 + p:2 + p + s]
    assert (seq[0], seq[1], seq[2 + s]) == (fh.PRE, fh.SUF, fh.MID)
    return seq[3 + s:3 + s + p], seq[3 + s + p:3 + s + p + m], seq[2:2 + s]


def test_the_document_comes_back_at_token_level(tok):
    docs = mh.synth_batch([0, 1, 2, 3, 50, 300], seed=2)[0] * 4
    for eot in (None, fh.EOT):
        seqs, labels, info = tok.fim_tokens(docs, **SENT, eot=eot, fim_rate=0.7, seed=5)
        assert {i[0] for i in info} == {0, 1, 2}
        for ids, seq, lab, inf in zip(docs, seqs, labels, info):
            P, M, S = split(seq, inf, eot)
            assert P + M + S == ids and lab == seq


def test_the_document_comes_back_at_character_level(tok):
    docs = list(fh.encode_docs())
    seed = fh.encode_seed(tok, docs, fim_rate=0.8)
    cuts = tok.fim_cuts(docs, fim_rate=0.8, seed=seed)
    rows, labels, lengths, info = tok.encode_batch_fim(docs, level="char", **SENT, eot=fh.EOT, fim_rate=0.8, seed=seed)
    assert len({len(r) for r in rows}) == 1 and [i[0] for i in info] == [c[0] for c in cuts]
    for text, row, n, inf, (mode, a, b) in zip(docs, rows, lengths, info, cuts):
        P, M, S = split(row[:n], inf, fh.EOT)
        t = tok.normalize(text)
        assert tok.decode(P) + tok.decode(M) + tok.decode(S) == t
        assert (tok.decode(P), tok.decode(M)) == (t[:a], t[a:b])
    # a special under a cut is plain text in both pieces, one inside a piece is a special
    mask_id = tok.get_vocab()["[MASK]"]
    under = [k for k, (t, (mode, a, b)) in enumerate(zip(docs, cuts)) if mode and fh.special_hits(tok, t, a, b) == (True, False)]
    whole = [k for k, (t, (mode, a, b)) in enumerate(zip(docs, cuts)) if mode and "[MASK]" in t and fh.special_hits(tok, t, a, b) == (False, True)]
    assert under and whole
    assert all(mask_id not in rows[k] for k in under if "[MASK]" in docs[k] and docs[k].count("[") == 1)
    assert all(mask_id in rows[k] for k in whole)


def test_token_level_rows_are_fim_tokens_of_the_encoded_batch(tok):
    docs = list(fh.encode_docs())[:20]
    rows, labels, lengths, info = tok.encode_batch_fim(docs, 24, level="token", **SENT, seed=3, bos_id=1, pad_id=0, loss="middle")
    seqs, labs, inf = tok.fim_tokens(tok.encode_batch(docs), **SENT, seed=3, max_length=23, loss="middle")
    assert info == inf
    for row, lab, n, seq, sl in zip(rows, labels, lengths, seqs, labs):
        assert row == [1] + seq + [0] * (23 - len(seq)) and lab == [-100] + sl + [-100] * (23 - len(seq)) and n == len(seq) + 1


def test_a_slice_under_a_shifted_first_doc(tok):
    docs = mh.synth_batch([5, 0, 40, 3, 300, 1, 17, 9], seed=4)[0]
    kw = {**SENT, "eot": fh.EOT, "seed": 8, "max_length": 30, "loss": "middle"}
    whole = tok.fim_tokens(docs, first_doc=1 << 40, **kw)
    part = tok.fim_tokens(docs[3:7], first_doc=(1 << 40) + 3, **kw)
    assert all(w[3:7] == p for w, p in zip(whole, part))
    texts = list(fh.encode_docs())[:12]
    cuts = tok.fim_cuts(texts, seed=8, first_doc=5)
    assert tok.fim_cuts(texts[4:9], seed=8, first_doc=9) == cuts[4:9]
    whole = tok.encode_batch_fim(texts, 40, **SENT, seed=8, first_doc=5)
    part = tok.encode_batch_fim(texts[4:9], 40, **SENT, seed=8, first_doc=9)
    assert all(w[4:9] == p for w, p in zip(whole, part))


def test_labels_of_both_loss_modes(tok):
    docs = mh.synth_batch([12, 0, 40, 3, 7] * 3, seed=6)[0]
    for eot in (None, fh.EOT):
        seqs, all_labels, info = tok.fim_tokens(docs, **SENT, eot=eot, seed=2, loss="all")
        seqs2, mid_labels, info2 = tok.fim_tokens(docs, **SENT, eot=eot, seed=2, loss="middle")
        assert seqs == seqs2 == all_labels and info == info2 and {i[0] for i in info} == {0, 1, 2}
        for seq, lab, (mode, p, m, s) in zip(seqs, mid_labels, info):
            if mode == 0:
                assert lab == seq
                continue
            first = 3 + p + s  # both orders end with the middle
            assert lab[:first] == [-100] * first and lab[first:] == seq[first:] and len(seq) - first == m + (eot is not None)


def test_sentinels_by_string_and_refused_arguments(tok):
    docs = [[1, 2, 3, 4, 5, 6]]
    v = tok.get_vocab()
    by_name = tok.fim_tokens(docs, pre="[MASK]", suf="[PAD]", mid="<|endoftext|>", eot="[PAD]", fim_rate=1)
    assert by_name == tok.fim_tokens(docs, pre=v["[MASK]"], suf=v["[PAD]"], mid=v["<|endoftext|>"], eot=v["[PAD]"], fim_rate=1)
    for bad, words in (({"fim_rate": 1.5}, "[0, 1]"), ({"spm_rate": -0.1}, "[0, 1]"), ({"max_length": 3}, "max_len 0 or above 3"),
                       ({"max_length": 4, "eot": 7}, "max_len 0 or above 4"), ({"max_length": 0}, "max_len 0 or above 3"), ({"loss": "some"}, "loss"),
                       ({"pre": "nope"}, "special token"), ({"mid": None}, "mid"), ({"suf": 1 << 32}, "2^32"), ({"seed": -1}, "seed"),
                       ({"first_doc": 1 << 64}, "first_doc")):
        with pytest.raises(ValueError) as e:
            tok.fim_tokens(docs, **{**SENT, **bad})
        assert words in str(e.value), (bad, str(e.value))
    assert sum(tok.fim_tokens(docs, **SENT, max_length=4, fim_rate=1)[2][0][1:]) == 1  # the smallest max_length: one id of content
    with pytest.raises(ValueError):
        tok.encode_batch_fim(["a b c"], level="word", **SENT)
    with pytest.raises(ValueError):
        tok.encode_batch_fim(["a b c"], 4, bos_id=1, **SENT)  # three slots of content: the sentinels alone need them
    with pytest.raises(ValueError):
        tok.fim_cuts(["a"], fim_rate=2)
    assert tok.encode_batch_fim([], **SENT) == ([], [], [], [])


def test_statistical_contract():
    from yet_another_bpe.tokenizer import BBPETokenizer

    n = 20_000
    for fim_rate, spm_rate, seed in ((0.5, 0.5, 21), (0.9, 0.25, 22)):
        Tf, Ts = fh.threshold(fim_rate), fh.threshold(spm_rate)
        modes = [BBPETokenizer._fim_draw(seed, d, 10, Tf, Ts)[0] for d in range(n)]
        fim, spm = sum(m != 0 for m in modes), sum(m == 2 for m in modes)
        q, qs = Tf / 2**32, Ts / 2**32
        bound, bound_spm = 5 * math.sqrt(n * q * (1 - q)), 5 * math.sqrt(fim * qs * (1 - qs))
        print(f"fim_rate {fim_rate}: {fim} of {n} transformed, allowed {n * q:.0f} +- {bound:.0f}; spm_rate {spm_rate}: {spm} of {fim} SPM, "
              f"allowed {fim * qs:.0f} +- {bound_spm:.0f}")
        assert abs(fim - n * q) <= bound and abs(spm - fim * qs) <= bound_spm
    # and the cut points are the draws the docstring states: a <= b <= n, both ends reached
    cuts = [BBPETokenizer._fim_draw(5, d, 3, 1 << 32, 0)[1:] for d in range(2000)]
    assert all(0 <= a <= b <= 3 for a, b in cuts) and {(0, 0), (0, 3), (3, 3), (1, 2)} <= set(cuts)
