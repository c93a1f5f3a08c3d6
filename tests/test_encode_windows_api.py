"""CPU: the contract of the overlapping windows, BBPETokenizer.encode_batch_windows, against a brute-force formulation written
here -- row by row, slot by slot over encode_batch's and encode_with_offsets' output -- on G9's set-ups and hand-made documents:
BOS / EOS, both padding sides, strides from none to all but one id, the spans of the slots, every ValueError (from the device
form too, which validates before any device work) and the shapes of an empty batch."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from tests import encode_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

IDENT = {bytes([i]): i for i in range(256)}
HAND = ["", "a", "ab cd", "", "the quick brown fox jumps over the lazy dog", "é中\U0001F600", "x" * 40, ""]
FRAMES = list(itertools.product((None, 4_000_000_000), (None, 0)))  # (bos, eos): ids no vocab holds, and id 0
PAD = 77_777


def brute(enc, spans, L, stride, bos, eos, side):
    """enc[d]: the ids of document d, spans[d]: their (start, end) -> the five results"""
    n_added = (bos is not None) + (eos is not None)
    C = L - n_added
    rows, row_doc, row_start, lengths, offs = [], [], [], [], []
    for d, e in enumerate(enc):
        n_rows = 1 if len(e) <= C else 1 + -(-(len(e) - C) // (C - stride))
        for k in range(n_rows):
            s = k * (C - stride)
            kept = min(C, len(e) - s) + n_added
            row, off = [], []
            for col in range(L):
                p = col - (L - kept) if side == "left" else col  # the slot's index into the row's sequence
                if p < 0 or p >= kept:
                    row.append(PAD), off.append((0, 0))
                elif bos is not None and p == 0:
                    row.append(bos), off.append((0, 0))
                elif eos is not None and p == kept - 1:
                    row.append(eos), off.append((0, 0))
                else:
                    j = s + p - (bos is not None)
                    row.append(e[j]), off.append(tuple(spans[d][j]))
            rows.append(row), row_doc.append(d), row_start.append(s), lengths.append(kept), offs.append(off)
    return rows, row_doc, row_start, lengths, offs


def check(tok, texts, what):
    enc = tok.encode_batch(texts)
    longest = max([len(e) for e in enc], default=0)
    for unit in ("char", "byte"):
        with_off = [tok.encode_with_offsets(t, unit) for t in texts]
        assert [ids for ids, _ in with_off] == enc
        spans = [sp for _, sp in with_off]
        for bos, eos in FRAMES:
            n_added = (bos is not None) + (eos is not None)
            for L in sorted({n_added + 1, n_added + 2, 5, 16, longest + n_added, longest + n_added + 2}):
                C = L - n_added
                if C < 1:
                    continue
                for stride, side in itertools.product(sorted({0, 1, C // 2, C - 1} & set(range(C))), ("right", "left")):
                    kw = dict(pad_id=PAD, bos_id=bos, eos_id=eos, padding_side=side)
                    exp = brute(enc, spans, L, stride, bos, eos, side)
                    assert tok.encode_batch_windows(texts, L, stride, offsets=unit, **kw) == exp, (what, unit, L, stride, bos, eos, side)
                    if unit == "char":
                        assert tok.encode_batch_windows(texts, L, stride, **kw) == exp[:4], (what, L, stride, bos, eos, side)


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups:
        check(tok, g9["texts"][:24], name)


def test_hand_made_documents():
    tok = BBPETokenizer(vocab={**IDENT, b"ab": 256, b"th": 257, b"<s>": 258}, merges=[(b"a", b"b"), (b"t", b"h")], special_tokens=["<s>", "<t>"])
    check(tok, HAND, "hand-made")
    check(tok, ["", ""], "only empty documents")
    check(tok, ["<t>", "<s>", "<t><t>"], "specials with and without an id")
    check(tok, ["abab"], "one document")
    # every document has a row, an empty one included; the last row is the first that reaches the end
    assert tok.encode_batch_windows(["", "xyz"], 2, pad_id=9) == ([[9, 9], [120, 121], [122, 9]], [0, 1, 1], [0, 0, 2], [0, 2, 1])
    assert tok.encode_batch_windows(["wxyz"], 3, 2, pad_id=9) == ([[119, 120, 121], [120, 121, 122]], [0, 0], [0, 1], [3, 3])
    assert tok.encode_batch_windows(["wxyz"], 4, 1, pad_id=9, bos_id=1, padding_side="left") == (
        [[1, 119, 120, 121], [9, 1, 121, 122]], [0, 0], [0, 2], [4, 3])
    assert tok.encode_batch_windows(["xy"], 3, eos_id=2, offsets="byte", pad_id=9)[4] == [[(0, 1), (1, 2), (0, 0)]]


def test_stride_0_equals_padded_when_nothing_overflows(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups[:2]:
        texts = g9["texts"][:24]
        L = max(len(e) for e in tok.encode_batch(texts)) + 1
        for side in ("right", "left"):
            rows, row_doc, row_start, lengths = tok.encode_batch_windows(texts, L, padding_side=side, pad_id=PAD)
            assert (rows, lengths) == tok.encode_batch_padded(texts, L, padding_side=side, pad_id=PAD), (name, side)
            assert row_doc == list(range(len(texts))) and row_start == [0] * len(texts)


def test_empty_texts_shapes():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    assert tok.encode_batch_windows([], 8, 2) == ([], [], [], [])
    assert tok.encode_batch_windows([], 8, 2, offsets="char") == ([], [], [], [], [])
    for unit in (None, "byte"):  # the device form answers without a device: no texts, no device work
        out = tok.encode_array_windows([], 8, 2, offsets=unit)
        assert [(a.shape, a.dtype) for a in out[:4]] == [((0, 8), np.uint32)] + [((0,), np.uint32)] * 3
        assert len(out) == (4 if unit is None else 5) and (unit is None or (out[4].shape, out[4].dtype) == ((0, 8, 2), np.uint64))


def test_value_errors():
    tok = BBPETokenizer(vocab=dict(IDENT), merges=[])
    bad = [{"max_length": 4.0}, {"max_length": "4"}, {"max_length": None}, {"max_length": 0}, {"max_length": -2},
           {"max_length": 1, "bos_id": 1}, {"max_length": 2, "bos_id": 1, "eos_id": 2},                      # max_length <= n_added
           {"stride": 4}, {"stride": -1}, {"stride": 1.0}, {"stride": None}, {"stride": 3, "eos_id": 2},       # not in [0, C - 1]
           {"stride": 2, "bos_id": 1, "eos_id": 2},
           {"padding_side": "up"}, {"padding_side": None}, {"offsets": "word"}, {"offsets": True},
           {"pad_id": -1}, {"bos_id": 1 << 32}, {"eos_id": 1.5}, {"pad_id": "7"},
           {"offsets": "char", "dropout": 0.1}, {"offsets": "byte", "dropout": 1.0},
           {"dropout": -0.5}, {"dropout": 0.1, "seed": -1}]
    for kw in bad:
        kw = {"max_length": 4, **kw}
        for call in (tok.encode_batch_windows, tok.encode_array_windows):  # (the device form: before any device work)
            with pytest.raises(ValueError):
                call(["abcdef"], **kw)
    assert tok.encode_batch_windows(["abc"], 4, 3)[1] == [0] and tok.encode_batch_windows(["abc"], 2, 0, bos_id=(1 << 32) - 1)[3] == [2, 2, 2]
    assert tok.encode_batch_windows(["abc"], 4, offsets="char", dropout=0.0)[4] == [[(0, 1), (1, 2), (2, 3), (0, 0)]]
