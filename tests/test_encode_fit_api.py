"""CPU: the contract of the whole-document packing, BBPETokenizer.encode_batch_fit: a hand-written example, the properties any
result has (every sequence whole and exactly once, documents of one length dealt in ascending order, rows in descending shape
order, the rooms of a literal best-fit decreasing) on G9's set-ups, BOS / EOS that survive the cut, empty documents, dropout,
the default pad id and every ValueError."""
from __future__ import annotations

import itertools
from collections import Counter

import pytest

from tests import encode_helpers
from tests import fit_helpers as fh
from yet_another_bpe.tokenizer import BBPETokenizer

IDENT = {bytes([i]): i for i in range(256)}
FRAMES = list(itertools.product((None, 4_000_000_000), (None, 0)))  # (bos, eos): ids no vocab holds, and id 0
NO_DOC = 0xFFFFFFFF


def check(tok, texts, what, **enc):
    pad = 77_777
    content = tok._encode_batch_for_layout(texts, enc.get("dropout", 0.0), enc.get("seed", 0))
    for (bos, eos), C in itertools.product(FRAMES, (2, 3, 7, 16, 64)):
        n_added = (bos is not None) + (eos is not None)
        seqs = [([bos] if bos is not None else []) + e[:C - n_added] + ([eos] if eos is not None else []) for e in content]
        ids, doc, pos, used = tok.encode_batch_fit(texts, C, pad_id=pad, bos_id=bos, eos_id=eos, **enc)
        assert len(ids) == len(doc) == len(pos) == len(used) and all(len(r) == C for r in ids + doc + pos), (what, C)
        placed, shapes = [], []
        for ri, rd, rp, u in zip(ids, doc, pos, used):
            assert rd[u:] == [NO_DOC] * (C - u) and ri[u:] == [pad] * (C - u) and rp[u:] == [0] * (C - u), (what, C)
            row_docs, c = [], 0
            while c < u:  # the sequences of the row, end to end and whole
                d = rd[c]
                n = len(seqs[d])
                assert n and ri[c:c + n] == seqs[d] and rd[c:c + n] == [d] * n and rp[c:c + n] == list(range(n)), (what, C, d)
                row_docs.append(d)
                c += n
            assert c == u
            placed += row_docs
            shapes.append(tuple(len(seqs[d]) for d in row_docs))
        assert sorted(placed) == [d for d, s in enumerate(seqs) if s], (what, C)  # each exactly once, the empty ones nowhere
        assert shapes == sorted(shapes, reverse=True) and all(list(s) == sorted(s, reverse=True) for s in shapes), (what, C)
        by_len: dict[int, list[int]] = {}
        for d in placed:  # row by row, left to right: the documents of one length ascend
            by_len.setdefault(len(seqs[d]), []).append(d)
        assert all(v == sorted(v) for v in by_len.values()), (what, C)
        assert Counter(C - sum(s) for s in shapes) == fh.literal_rooms([len(s) for s in seqs], C), (what, C)
        assert sum(1 for s in shapes if 2 * sum(s) <= C) <= 1, (what, C)


def test_hand_example():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    texts = ["aaaaaa", "bbbbbb", "cccccc", "dd", "ee", "ff"]  # lengths 6, 6, 6, 2, 2, 2 in rows of 10: (6, 2, 2), (6, 2), (6)
    ids, doc, pos, used = tok.encode_batch_fit(texts, 10, pad_id=0)
    a, b, c, d, e, f = (ord(ch) for ch in "abcdef")
    assert ids == [[a] * 6 + [d] * 2 + [e] * 2, [b] * 6 + [f] * 2 + [0] * 2, [c] * 6 + [0] * 4]
    assert doc == [[0] * 6 + [3] * 2 + [4] * 2, [1] * 6 + [5] * 2 + [NO_DOC] * 2, [2] * 6 + [NO_DOC] * 4]
    assert pos == [list(range(6)) + [0, 1] * 2, list(range(6)) + [0, 1, 0, 0], list(range(6)) + [0] * 4]
    assert used == [10, 8, 6]
    # the three-way split of one shape: 5 rows of (5,) and 5 sequences of 2 in rows of 9 -> two full rows, one partial, two untouched
    ids, doc, pos, used = tok.encode_batch_fit(["vwxyz"] * 5 + ["ab"] * 5, 9, pad_id=0)
    assert [[x for k, x in enumerate(r) if k == 0 or r[k - 1] != x] for r in doc] == [[0, 5, 6], [1, 7, 8], [2, 9, NO_DOC], [3, NO_DOC], [4, NO_DOC]]
    assert used == [9, 9, 7, 5, 5]


def test_bos_and_eos_survive_the_cut():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    x, y = ord("x"), ord("y")
    assert tok.encode_batch_fit(["xyxyxyx"], 4, bos_id=1, eos_id=2) == ([[1, x, y, 2]], [[0] * 4], [[0, 1, 2, 3]], [4])
    assert tok.encode_batch_fit(["xyxyxyx", "y"], 2, bos_id=1, eos_id=2) == ([[1, 2], [1, 2]], [[0, 0], [1, 1]], [[0, 1], [0, 1]], [2, 2])
    assert tok.encode_batch_fit(["xyx"], 2, eos_id=2)[0] == [[x, 2]] and tok.encode_batch_fit(["xyx"], 1, bos_id=1)[0] == [[1]]
    assert tok.encode_batch_fit(["xyx", "xy"], 5, eos_id=2, pad_id=9) == ([[x, y, x, 2, 9], [x, y, 2, 9, 9]], [[0] * 4 + [NO_DOC], [1] * 3 + [NO_DOC] * 2],
                                                                     [[0, 1, 2, 3, 0], [0, 1, 2, 0, 0]], [4, 3])


def test_empty_documents_vanish():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    assert tok.encode_batch_fit([], 4) == ([], [], [], []) and tok.encode_batch_fit(["", ""], 4) == ([], [], [], [])
    assert tok.encode_batch_fit(["", "ab", "", "c"], 4, pad_id=7) == ([[97, 98, 99, 7]], [[1, 1, 3, NO_DOC]], [[0, 1, 0, 0]], [3])
    # with BOS or EOS an empty document is a sequence of its own
    assert tok.encode_batch_fit(["", "ab", ""], 4, eos_id=5, pad_id=7) == ([[97, 98, 5, 5], [5, 7, 7, 7]], [[1, 1, 1, 0], [2] + [NO_DOC] * 3],
                                                                        [[0, 1, 2, 0], [0, 0, 0, 0]], [4, 1])


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups:
        check(tok, g9["texts"][:24], name)
    tok = setups[0][2]
    check(tok, g9["texts"][:24], "dropout", dropout=0.3, seed=11)
    assert tok.encode_batch_fit(g9["texts"][:24], 16, dropout=0.3, seed=11) != tok.encode_batch_fit(g9["texts"][:24], 16)


def test_pad_id_default():
    with_pad = BBPETokenizer(vocab={**IDENT, b"[PAD]": 300}, merges=[])
    without = BBPETokenizer(vocab=dict(IDENT), merges=[])
    assert with_pad.encode_batch_fit(["abc"], 4)[0] == [[97, 98, 99, 300]] and without.encode_batch_fit(["abc"], 4)[0] == [[97, 98, 99, 0]]
    assert with_pad.encode_batch_fit(["abc"], 4, pad_id=0)[0] == [[97, 98, 99, 0]]  # an explicit 0 is 0


def test_value_errors():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    for call in (tok.encode_batch_fit, tok.encode_array_fit):  # the device form validates before any device work
        for name in ("pad_id", "bos_id", "eos_id"):
            for bad in (-1, 1 << 32, 1.5, "7"):
                with pytest.raises(ValueError):
                    call(["a"], 4, **{name: bad})
        for bad in (0, -3, 2.5, "8", None):
            with pytest.raises(ValueError):
                call(["a"], bad)
        with pytest.raises(ValueError):
            call(["a"], 1, bos_id=1, eos_id=2)  # seq_len < n_added
        with pytest.raises(ValueError):
            call(["a"], 0, eos_id=2)
        for bad in (-0.1, 1.5, "x"):
            with pytest.raises(ValueError):
                call(["a"], 4, dropout=bad)
        with pytest.raises(ValueError):
            call(["a"], 4, dropout=0.5, seed=-1)
    for name in ("pad_id", "bos_id", "eos_id"):
        assert tok.encode_batch_fit(["a"], 4, **{name: (1 << 32) - 1})[3] in ([1], [2])
    assert tok.encode_batch_fit(["a"], 1, eos_id=2) == ([[2]], [[0]], [[0]], [1]) and tok.encode_batch_fit(["a"], 2, bos_id=1, eos_id=2)[0] == [[1, 2]]
