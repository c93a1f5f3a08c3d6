"""GPU: BBPETokenizer.encode_array_span_corrupted (yabpe_encode_words, yabpe_span_corrupt, then yabpe_layout_pad over the
inputs and over the targets) against the plain-Python encode_batch_span_corrupted, on tests/golden/corpus.en cut into
documents with specials between and inside them: under the default split pattern, "cl100k", "o200k_base" and digit_group =
3, per token and per word, max_tokens below, at and above the document lengths, both row lengths given and left open, BOS
and EOS, both truncation and padding sides, no texts and empty texts."""
from __future__ import annotations

import itertools
from functools import lru_cache

import numpy as np
import pytest

from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu
BOS, EOS = 70001, 70002
SENT = ["[MASK]", "[PAD]", "<|endoftext|>"] + list(range(80000, 80020))  # specials by name, then plain ids
OPTIONS = [{}, {"pretokenizer": "cl100k"}, {"pretokenizer": "o200k_base"}, {"digit_group": 3}]


@lru_cache(maxsize=None)
def docs() -> tuple[str, ...]:
    """corpus.en in documents of 0 to 400 words (one of them longer than a block of 256 ids by far), a special between the
    halves of every third one, a document of specials only, the special without an id, numbers for digit_group"""
    words = mh.corpus_words()
    sizes = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 400, 0, 7, 30, 61, 2, 0]
    out, at = [], 0
    for k, n in enumerate(sizes):
        w = words[at:at + n]
        at += n
        text = " ".join(w[:n // 2]) + ("<|endoftext|>" if k % 3 == 0 and n else " ") + " ".join(w[n // 2:])
        out.append(text.strip() if n else "")
    out += ["<|endoftext|>[MASK]<|endoftext|>", f"a {mh.NO_ID} b{mh.NO_ID}c 1234567 89012.50 x", mh.NO_ID]
    return tuple(out)


@lru_cache(maxsize=None)
def tokenizer(index: int):
    return mh.tokenizer(**OPTIONS[index])


@lru_cache(maxsize=None)
def doc_lengths(index: int) -> tuple[int, ...]:
    return tuple(len(e[0]) for e in tokenizer(index).encode_batch_with_words(list(docs())))


def check(tok, texts, max_length, max_target_length, **kw):
    exp = tok.encode_batch_span_corrupted(texts, max_length, max_target_length, **kw)
    got = tok.encode_array_span_corrupted(texts, max_length, max_target_length, **kw)
    assert [g.dtype for g in got] == [np.uint32, np.int32, np.uint32, np.uint32]
    assert got[0].shape == (len(texts), len(exp[0][0])) and got[1].shape == (len(texts), len(exp[1][0]))
    assert [g.tolist() for g in got] == [list(e) for e in exp], (max_length, max_target_length, kw)
    return got


@pytest.mark.parametrize("index", range(len(OPTIONS)), ids=[str(o) for o in OPTIONS])
def test_matches_plain_python(index):
    tok, texts = tokenizer(index), list(docs())
    lens = doc_lengths(index)
    assert max(lens) > 300 and 0 in lens
    at = sorted(set(lens))[len(set(lens)) // 2]  # a length some document has: max_tokens at it, below all but the shortest, above all
    for whole_word, max_tokens in itertools.product((False, True), (None, 2, at, max(lens) + 5)):
        kw = {"sentinels": SENT, "p": 0.3, "seed": 21, "first_doc": 3, "whole_word": whole_word, "max_tokens": max_tokens}
        rows, labels, lengths, label_lengths = check(tok, texts, None, None, **kw)
        assert rows.shape[1] == lengths.max() and labels.shape[1] == label_lengths.max()
        check(tok, texts, 24, 12, bos_id=BOS, eos_id=EOS, **kw)
    kw = {"sentinels": SENT, "p": 0.5, "mean_span_length": 2.0, "max_span_length": 5, "seed": 4}
    for (bos, eos), trunc, side in itertools.product(((BOS, None), (None, EOS)), ("right", "left"), ("right", "left")):
        rows, labels, lengths, label_lengths = check(tok, texts, 16, 40, bos_id=bos, eos_id=eos, truncation=trunc, padding_side=side,
                                                     final_sentinel=side == "left", **kw)
        # labels are -100 outside the content of the row: in BOS, EOS and pad slots
        for d in range(len(texts)):
            n = int(label_lengths[d])
            lo = labels.shape[1] - n if side == "left" else 0
            content = range(lo + (bos is not None), lo + n - (eos is not None))
            assert all(labels[d, c] == mh.IGNORE for c in range(labels.shape[1]) if c not in content)
            assert all(labels[d, c] >= 0 for c in content)


def test_the_draws_do_not_depend_on_the_rows_or_the_batch():
    tok, texts = tokenizer(0), list(docs())
    kw = {"sentinels": SENT, "p": 0.4, "seed": 2}
    full = tok.encode_array_span_corrupted(texts, **kw)
    cut = tok.encode_array_span_corrupted(texts, 8, 6, **kw)
    assert np.array_equal(cut[0], full[0][:, :8]) and np.array_equal(cut[1], full[1][:, :6])
    part = tok.encode_array_span_corrupted(texts[10:14], first_doc=10, **kw)  # a shard of the batch
    assert np.array_equal(part[2], full[2][10:14]) and np.array_equal(part[3], full[3][10:14]) and part[2].max() > 256
    for g, f, n in zip(part[:2], full[:2], part[2:]):  # (the shard's rows are as wide as its own longest sequence)
        assert all(np.array_equal(g[d, :n[d]], f[10 + d, :n[d]]) for d in range(4))


def test_p_zero_is_the_padded_batch():
    tok, texts = tokenizer(0), list(docs())
    rows, labels, lengths, label_lengths = tok.encode_array_span_corrupted(texts, 20, None, sentinels=SENT, p=0, bos_id=BOS)
    plain_rows, plain_len = tok.encode_array_padded(texts, 20, bos_id=BOS)
    assert np.array_equal(rows, plain_rows) and np.array_equal(lengths, plain_len)
    first = tok._vocab[b"[MASK]"]  # no runs: the targets are the final sentinel alone, sentinels[0], where the document has ids
    assert labels.shape == (len(texts), 2) and label_lengths.tolist() == [2 if n else 1 for n in doc_lengths(0)]
    assert all(labels[d].tolist() == ([mh.IGNORE, first] if n else [mh.IGNORE, mh.IGNORE]) for d, n in enumerate(doc_lengths(0)))


def test_no_texts_and_empty_texts():
    tok = tokenizer(0)
    for max_length, max_target in ((None, None), (8, 5)):
        rows, labels, lengths, label_lengths = tok.encode_array_span_corrupted([], max_length, max_target, sentinels=SENT)
        assert rows.shape == (0, max_length or 0) and labels.shape == (0, max_target or 0) and lengths.shape == label_lengths.shape == (0,)
        assert [x.dtype for x in (rows, labels, lengths, label_lengths)] == [np.uint32, np.int32, np.uint32, np.uint32]
    rows, labels, lengths, label_lengths = tok.encode_array_span_corrupted(["", ""], sentinels=SENT)
    assert rows.shape == labels.shape == (2, 0) and lengths.tolist() == label_lengths.tolist() == [0, 0] and labels.dtype == np.int32
    rows, labels, lengths, label_lengths = tok.encode_array_span_corrupted(["", ""], 4, 0, sentinels=SENT, p=1)
    assert rows.shape == (2, 4) and labels.shape == (2, 0) and label_lengths.tolist() == [0, 0]
    rows, labels, lengths, label_lengths = tok.encode_array_span_corrupted(["", "a"], 3, 3, sentinels=SENT, p=1, bos_id=BOS)
    pad, s0, s1 = tok._vocab[b"[PAD]"], tok._vocab[b"[MASK]"], tok._vocab[b"[PAD]"]
    assert rows.tolist() == [[BOS, pad, pad], [BOS, s0, pad]] and lengths.tolist() == [1, 2]
    assert labels[0].tolist() == [mh.IGNORE] * 3 and labels[1, 0] == mh.IGNORE and labels[1, 1] == s0 and label_lengths.tolist() == [1, 3]
    assert labels[1, 2] == tok.encode("a")[0]
    with pytest.raises(ValueError):
        tok.encode_array_span_corrupted(["a"], sentinels=[])
