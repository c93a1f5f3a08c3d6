"""GPU: BBPETokenizer.encode_array_fim (at character level yabpe_fim_cuts, one yabpe_encode over the 3 n pieces and yabpe_fim
with pieces; at token level yabpe_encode and yabpe_fim; then yabpe_layout_pad over the sequences and over the labels) against
the plain-Python encode_batch_fim with the corpus.en model of tests/mask_helpers.py: texts that hold special tokens inside
pieces and under a cut, a lowercase NFC model whose text changes length under the front, the cl100k pattern with digit_group
= 3 where a cut inside a digit run regroups the digits, max_length left open and small, and an empty batch."""
from __future__ import annotations

import itertools
import unicodedata

import numpy as np
import pytest

from tests import fim_helpers as fh
from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu
BOS, EOS = 70001, 70002
SENT = {"pre": "[MASK]", "suf": "[PAD]", "mid": 80000}


def check(tok, texts, max_length, **kw):
    exp = tok.encode_batch_fim(texts, max_length, **kw)
    got = tok.encode_array_fim(texts, max_length, **kw)
    assert [g.dtype for g in got] == [np.uint32, np.int32, np.uint32, np.uint32]
    assert got[0].shape == got[1].shape == (len(texts), len(exp[0][0]) if texts else (max_length or 0)) and got[3].shape == (len(texts), 4)
    assert [g.tolist() for g in got[:3]] == [list(e) for e in exp[:3]] and [tuple(r) for r in got[3].tolist()] == exp[3], (max_length, kw)
    return got


def test_both_levels_match_plain_python():
    tok, texts = mh.tokenizer(), list(fh.encode_docs())
    seed = fh.encode_seed(tok, texts, fim_rate=0.8)
    cuts = tok.fim_cuts(texts, fim_rate=0.8, seed=seed)
    hits = [fh.special_hits(tok, t, a, b) for t, (mode, a, b) in zip(texts, cuts) if mode]
    assert any(h[0] for h in hits) and any(h[1] for h in hits)  # a special under a cut, and one inside a piece
    for level, (max_length, eot, loss) in itertools.product(("char", "token"), ((None, None, "all"), (12, "<|endoftext|>", "middle"), (300, 80001, "all"))):
        rows, labels, lengths, info = check(tok, texts, max_length, level=level, fim_rate=0.8, seed=seed, eot=eot, loss=loss, **SENT)
        assert {int(m) for m in info[:, 0]} == {0, 1, 2}
        if max_length is None:
            assert rows.shape[1] == lengths.max() > 256
    for (bos, eos), side in itertools.product(((BOS, None), (None, EOS), (BOS, EOS)), ("right", "left")):
        rows, labels, lengths, _info = check(tok, texts, 16, level="char", seed=seed + 1, first_doc=1 << 40, bos_id=bos, eos_id=eos, padding_side=side,
                                             truncation=side, loss="middle", eot=80001, **SENT)
        for d in range(len(texts)):  # labels are -100 in BOS, EOS and pad slots
            n = int(lengths[d])
            lo = rows.shape[1] - n if side == "left" else 0
            content = range(lo + (bos is not None), lo + n - (eos is not None))
            assert all(labels[d, c] == mh.IGNORE for c in range(rows.shape[1]) if c not in content)


def test_a_model_whose_text_changes_length_under_the_front():
    tok = mh.tokenizer(mh.SPECIALS_LOWER, lowercase=True, normalizer="nfc")
    texts = [unicodedata.normalize("NFD", "NAÏVE Café İstanbul [mask] Done") * 3, "", "Hello WORLD [pad] ÉÉ plain text", "İİİİ", "[mask]"] * 3
    assert any(len(tok.normalize(t)) != len(t) for t in texts)
    sent = {"pre": "[mask]", "suf": "[pad]", "mid": 80000}
    for level, max_length in itertools.product(("char", "token"), (None, 10)):
        check(tok, texts, max_length, level=level, fim_rate=0.9, seed=5, **sent)


def test_a_cut_inside_a_digit_run_regroups_the_digits():
    tok = mh.tokenizer(pretokenizer="cl100k", digit_group=3)
    texts = [f"In {1234567 + i} we paid {89012 + 7 * i}.50 for 00{i}" for i in range(30)] + ["1234567890123", ""]
    seed = next(s for s in range(200) if any(
        mode and 0 < a < len(t) and t[a - 1].isdigit() and t[a].isdigit() and
        tok._encode_normalized(t[:a]) + tok._encode_normalized(t[a:]) != tok._encode_normalized(t)
        for t, (mode, a, b) in zip(texts, tok.fim_cuts(texts, fim_rate=1, seed=s))))
    for level, max_length in itertools.product(("char", "token"), (None, 9)):
        check(tok, texts, max_length, level=level, fim_rate=1, seed=seed, eot="<|endoftext|>", **SENT)


def test_no_texts_and_empty_texts():
    tok = mh.tokenizer()
    for level, max_length in itertools.product(("char", "token"), (None, 8)):
        rows, labels, lengths, info = check(tok, [], max_length, level=level, **SENT)
        assert rows.shape == (0, max_length or 0) and lengths.shape == (0,) and info.shape == (0, 4)
        rows, labels, lengths, info = check(tok, ["", ""], max_length, level=level, fim_rate=1, **SENT)
        assert lengths.tolist() == [3, 3] and info[:, 1:].tolist() == [[0, 0, 0]] * 2
        rows, labels, lengths, info = check(tok, ["", ""], max_length, level=level, fim_rate=0, **SENT)
        assert lengths.tolist() == [0, 0] and rows.shape == (2, max_length or 0)
    with pytest.raises(ValueError):
        tok.encode_array_fim(["a"], 3, **SENT)
    with pytest.raises(ValueError):
        tok.encode_array_fim(["a"], level="word", **SENT)
