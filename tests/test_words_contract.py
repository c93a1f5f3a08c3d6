"""CPU: BBPETokenizer.encode_with_words, the plain-Python contract of yabpe_encode_words -- the ids are encode's, and every id
names the piece of its document it was made from: the special occurrences and the matches of the split pattern, in order."""
from __future__ import annotations

import pytest

from tests import mask_helpers as mh


def pieces_of(tok, text):
    """[(piece bytes, is special)] of the normalised document, from the tokenizer's own patterns"""
    text = tok.normalize(text)
    out = []
    for part in ([text] if tok._special_pattern is None else tok._special_pattern.split(text)):
        if not part:
            continue
        if part in tok._special_set:
            out.append((part.encode("utf-8"), True))
        else:
            out += [(pre.encode("utf-8"), False) for pre in tok._pattern.findall(part)]
    return out


def check(tok, text):
    ids, words, special = tok.encode_with_words(text)
    assert ids == tok.encode(text)
    assert len(words) == len(special) == len(ids)
    assert all(a <= b for a, b in zip(words, words[1:]))
    pieces = pieces_of(tok, text)
    data = tok.normalize(text).encode("utf-8")
    assert b"".join(p for p, _ in pieces) == data  # the pieces tile the document
    bounds = [0]
    for p, _ in pieces:
        bounds.append(bounds[-1] + len(p))
    _ids, spans = tok.encode_with_offsets(text, unit="byte")
    for k, (w, sp) in enumerate(zip(words, special)):
        assert 0 <= w < len(pieces)
        assert sp == pieces[w][1]
        assert bounds[w] <= spans[k][0] and spans[k][1] <= bounds[w + 1]  # the id's bytes lie inside its piece
    for w, (piece, sp) in enumerate(pieces):
        mine = [k for k in range(len(ids)) if words[k] == w]
        if sp and piece not in tok._vocab:
            assert not mine  # a special without an id: an index nobody has
            continue
        assert mine == list(range(mine[0], mine[-1] + 1))
        assert (spans[mine[0]][0], spans[mine[-1]][1]) == (bounds[w], bounds[w + 1])  # together they cover exactly the piece
        if sp:
            assert len(mine) == 1 and ids[mine[0]] == tok._vocab[piece]
        elif all(tok._vocab_inv.get(ids[k]) is not None and ids[k] != tok._vocab.get(b"[UNK]", 0) for k in mine):
            assert b"".join(tok._vocab_inv[ids[k]] for k in mine) == piece  # the ids of one index decode to the piece
    return ids, words, special, pieces


def test_every_document_of_the_shared_set():
    tok = mh.tokenizer()
    docs = mh.word_docs()
    batch = tok.encode_batch_with_words(docs)
    assert len(batch) == len(docs)
    for text, got in zip(docs, batch):
        assert got == check(tok, text)[:3]
    assert tok.encode_with_words("") == ([], [], [])


def test_a_special_without_an_id_leaves_a_gap():
    tok = mh.tokenizer()
    ids, words, special, pieces = check(tok, f"a{mh.NO_ID}b{mh.NO_ID}{mh.NO_ID}c[MASK]")
    assert [p for p, _ in pieces] == [b"a", mh.NO_ID.encode(), b"b", mh.NO_ID.encode(), mh.NO_ID.encode(), b"c", b"[MASK]"]
    assert words == [0, 2, 5, 6] and special == [False, False, False, True]
    assert ids[-1] == tok._vocab[b"[MASK]"]
    assert tok.encode_with_words(mh.NO_ID) == ([], [], [])


def test_special_is_true_exactly_on_special_occurrences():
    tok = mh.tokenizer()
    text = "[PAD][PAD] pad [ MASK ] <|endoftext|>x<|endoftext|"
    ids, words, special, pieces = check(tok, text)
    assert [w for w, s in zip(words, special) if s] == [w for w, (_p, sp) in enumerate(pieces) if sp] == [0, 1, 7]
    assert sum(special) == 3


def test_a_piece_of_many_ids():
    tok = mh.tokenizer()
    ids, words, special, pieces = check(tok, "x" * 90 + " qzxjkv")
    assert len(pieces) == 2 and words.count(0) > 1 and words.count(1) > 1 and not any(special)


@pytest.mark.parametrize("options, specials, text", mh.OPTION_TEXTS, ids=[str(sorted(o)) for o, _s, _t in mh.OPTION_TEXTS])
def test_under_the_tokenizer_options(options, specials, text):
    tok = mh.tokenizer(specials, **options)
    ids, words, special, pieces = check(tok, text)
    assert ids and any(special)
    assert set(range(len(pieces))) - set(words)  # (every text holds the special without an id: a gap)
    plain = mh.tokenizer(specials)
    if "digit_group" in options:
        assert len(pieces) > len(pieces_of(plain, text))  # the digit runs are cut into more pieces
    if "lowercase" in options:
        assert b"".join(p for p, _ in pieces) == text.lower().encode("utf-8")
