"""CPU: the contract of the fixed-shape batches, BBPETokenizer.encode_batch_padded / encode_batch_packed, against a brute-force
formulation written here -- slot by slot over encode_batch's output -- on G9's set-ups and hand-made documents: every
combination of BOS / EOS, truncation side, padding side and drop_last, every ValueError, and the default pad id."""
from __future__ import annotations

import itertools

import pytest

from tests import encode_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

IDENT = {bytes([i]): i for i in range(256)}
HAND = ["", "a", "ab cd", "", "the quick brown fox jumps over the lazy dog", "é中\U0001F600", "x" * 40, ""]
FRAMES = list(itertools.product((None, 4_000_000_000), (None, 0)))  # (bos, eos): ids no vocab holds, and id 0


def seqs(tok, texts, bos, eos):
    return [([bos] if bos is not None else []) + ids + ([eos] if eos is not None else []) for ids in tok.encode_batch(texts)]


def brute_padded(tok, texts, L, pad, bos, eos, truncation, padding_side):
    n_added = (bos is not None) + (eos is not None)
    enc = tok.encode_batch(texts)
    if L is None:
        L = max([len(e) + n_added for e in enc], default=0)
    rows, lengths = [], []
    for e in enc:
        kept = min(len(e) + n_added, L)
        row = []
        for col in range(L):
            p = col - (L - kept) if padding_side == "left" else col  # the slot's index into the kept sequence
            if p < 0 or p >= kept:
                row.append(pad)
            elif bos is not None and p == 0:
                row.append(bos)
            elif eos is not None and p == kept - 1:
                row.append(eos)
            else:
                j = p - (bos is not None)  # index into the kept content
                row.append(e[j] if truncation == "right" else e[len(e) - (kept - n_added) + j])
        rows.append(row)
        lengths.append(kept)
    return rows, lengths


def brute_packed(tok, texts, L, pad, bos, eos, drop_last):
    ss = seqs(tok, texts, bos, eos)
    total = sum(len(s) for s in ss)
    n_rows = total // L if drop_last else (total + L - 1) // L
    ids = [[pad] * L for _ in range(n_rows)]
    doc = [[0xFFFFFFFF] * L for _ in range(n_rows)]
    pos = [[0] * L for _ in range(n_rows)]
    g = 0
    for d, s in enumerate(ss):
        for p, v in enumerate(s):
            if g < n_rows * L:
                ids[g // L][g % L], doc[g // L][g % L], pos[g // L][g % L] = v, d, p
            g += 1
    return ids, doc, pos


def check(tok, texts, what):
    pad = 77_777
    longest = max([len(e) for e in tok.encode_batch(texts)], default=0)
    for bos, eos in FRAMES:
        n_added = (bos is not None) + (eos is not None)
        for L in [None] + sorted({n_added, n_added + 1, 3, 5, longest, longest + n_added, longest + n_added + 2}):
            if L is not None and L < n_added:
                continue
            for tr, ps in itertools.product(("right", "left"), repeat=2):
                got = tok.encode_batch_padded(texts, L, pad_id=pad, bos_id=bos, eos_id=eos, truncation=tr, padding_side=ps)
                assert got == brute_padded(tok, texts, L, pad, bos, eos, tr, ps), (what, L, bos, eos, tr, ps)
        for L in (1, 2, 3, 7, 64):
            for dl in (False, True):
                got = tok.encode_batch_packed(texts, L, pad_id=pad, bos_id=bos, eos_id=eos, drop_last=dl)
                assert got == brute_packed(tok, texts, L, pad, bos, eos, dl), (what, L, bos, eos, dl)
                ids, doc, pos = got
                flat = [(i, d, p) for ri, rd, rp in zip(ids, doc, pos) for i, d, p in zip(ri, rd, rp)]
                if not dl:  # ids[doc == d] reassembles seq(d); pos counts it
                    for d, s in enumerate(seqs(tok, texts, bos, eos)):
                        assert [i for i, dd, _p in flat if dd == d] == s, (what, L, d)
                        assert [p for _i, dd, p in flat if dd == d] == list(range(len(s))), (what, L, d)
                    assert all(i == pad and p == 0 for i, dd, p in flat if dd == 0xFFFFFFFF)
    rows, lengths = tok.encode_batch_padded(texts)  # no truncation: the rows start with encode's ids
    for d, t in enumerate(texts):
        assert rows[d][:lengths[d]] == tok.encode(t) and set(rows[d][lengths[d]:]) <= {tok._vocab.get(b"[PAD]", 0)}, (what, d)


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups:
        check(tok, g9["texts"][:24], name)


def test_hand_made_documents():
    tok = BBPETokenizer(vocab={**IDENT, b"ab": 256, b"th": 257, b"<s>": 258}, merges=[(b"a", b"b"), (b"t", b"h")], special_tokens=["<s>", "<t>"])
    check(tok, HAND, "hand-made")
    check(tok, ["", ""], "only empty documents")
    check(tok, ["<t>", "<s>", "<t><t>"], "specials with and without an id")
    check(tok, [], "no documents")
    check(tok, ["abab"], "one document")
    assert tok.encode_batch_padded([], 5) == ([], []) and tok.encode_batch_padded([]) == ([], [])
    assert tok.encode_batch_packed([], 4) == ([], [], []) and tok.encode_batch_packed(["", ""], 4) == ([], [], [])  # an empty stream: no rows
    # BOS and EOS survive any cut, on both sides
    assert tok.encode_batch_padded(["abcdefg"], 2, bos_id=1, eos_id=2) == ([[1, 2]], [2])
    assert tok.encode_batch_padded(["xyz"], 3, bos_id=1, eos_id=2, truncation="left", padding_side="left") == ([[1, ord("z"), 2]], [3])
    assert tok.encode_batch_padded(["xyz", ""], 3, eos_id=2, padding_side="left", pad_id=9) == ([[ord("x"), ord("y"), 2], [9, 9, 2]], [3, 1])
    # a document with an empty seq contributes nothing; one with only BOS / EOS does
    assert tok.encode_batch_packed(["a", "", "b"], 2)[1] == [[0, 2]]
    assert tok.encode_batch_packed(["a", "", "b"], 2, eos_id=5) == ([[97, 5], [5, 98], [5, 0]], [[0, 0], [1, 2], [2, 0xFFFFFFFF]], [[0, 1], [0, 0], [1, 0]])


def test_pad_id_default():
    with_pad = BBPETokenizer(vocab={**IDENT, b"[PAD]": 300}, merges=[])
    without = BBPETokenizer(vocab=dict(IDENT), merges=[])
    assert with_pad.encode_batch_padded(["a", ""])[0] == [[97], [300]] and without.encode_batch_padded(["a", ""])[0] == [[97], [0]]
    assert with_pad.encode_batch_packed(["abc"], 2)[0] == [[97, 98], [99, 300]] and without.encode_batch_packed(["abc"], 2)[0] == [[97, 98], [99, 0]]
    assert with_pad.encode_batch_padded(["a", ""], pad_id=0)[0] == [[97], [0]]  # an explicit 0 is 0


def test_value_errors():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    for name in ("pad_id", "bos_id", "eos_id"):
        for bad in (-1, 1 << 32, 1.5, "7"):
            with pytest.raises(ValueError):
                tok.encode_batch_padded(["a"], 4, **{name: bad})
            with pytest.raises(ValueError):
                tok.encode_batch_packed(["a"], 4, **{name: bad})
        assert tok.encode_batch_padded(["a"], 4, **{name: (1 << 32) - 1})[1] in ([1], [2])
    for kw in ({"truncation": "middle"}, {"padding_side": "up"}, {"truncation": None}):
        with pytest.raises(ValueError):
            tok.encode_batch_padded(["a"], 4, **kw)
    with pytest.raises(ValueError):
        tok.encode_batch_padded(["a"], 1, bos_id=1, eos_id=2)  # max_length < n_added
    with pytest.raises(ValueError):
        tok.encode_batch_padded(["a"], 0, eos_id=2)
    with pytest.raises(ValueError):
        tok.encode_batch_padded(["a"], -1)
    assert tok.encode_batch_padded(["a"], 0) == ([[]], [0]) and tok.encode_batch_padded(["a"], 1, eos_id=2) == ([[2]], [1])
    for bad in (0, -3):
        with pytest.raises(ValueError):
            tok.encode_batch_packed(["a"], bad)
    # the device forms validate before any device work: the same errors without a GPU
    for call in (lambda: tok.encode_array_padded(["a"], 1, bos_id=1, eos_id=2), lambda: tok.encode_array_padded(["a"], 4, truncation="x"),
                 lambda: tok.encode_array_padded(["a"], 4, pad_id=-1), lambda: tok.encode_array_packed(["a"], 0),
                 lambda: tok.encode_array_packed(["a"], 4, eos_id=1 << 32)):
        with pytest.raises(ValueError):
            call()
