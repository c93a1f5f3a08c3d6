"""CPU: the contract of text pairs, BBPETokenizer.encode_batch_pairs: hand-written rows (the RoBERTa and the BERT form, ties with
odd and even C, windows), its two cross-checks against encode_batch_padded and encode_batch_windows, and every ValueError."""
from __future__ import annotations

import itertools

import pytest

from yet_another_bpe.tokenizer import BBPETokenizer

IDENT = {bytes([i]): i for i in range(256)}  # ids are bytes
HAND = ["", "a", "ab cd", "", "the quick brown fox jumps over the lazy dog", "é中\U0001F600", "x" * 40, ""]
PAD, BOS, EOS, SEP = 300, 301, 302, 303


@pytest.fixture(scope="module")
def tok():
    return BBPETokenizer(vocab={**IDENT, b"th": 256, b"he": 257}, merges=[(b"t", b"h"), (b"h", b"e")])


def ids_of(s: str) -> list[int]:
    return list(s.encode())


def test_roberta_form(tok):
    """<s> A </s></s> B </s>: two separators, EOS of its own"""
    rows, types, row_pair, row_start, first_len, second_len = tok.encode_batch_pairs(
        ["ab", "abcdef"], ["xyz", "uvwxyz"], 10, sep_id=SEP, n_sep=2, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    a, b, x, y, z = ids_of("abxyz")
    assert rows[0] == [BOS, a, b, SEP, SEP, x, y, z, EOS, PAD] and types[0] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 0]
    # C = 6 for 6 + 6 ids: three of each
    assert rows[1] == [BOS] + ids_of("abc") + [SEP, SEP] + ids_of("uvw") + [EOS] and types[1] == [0] * 6 + [1] * 4
    assert (row_pair, row_start, first_len, second_len) == ([0, 1], [0, 0], [2, 3], [3, 3])


def test_bert_form(tok):
    """[CLS] A [SEP] B [SEP]: the closing separator is the EOS, types 0 then 1"""
    rows, types, *_rest, first_len, second_len = tok.encode_batch_pairs(["abc"], ["de"], 9, sep_id=SEP, pad_id=PAD, bos_id=BOS, eos_id=SEP,
                                                                        padding_side="left")
    assert rows == [[PAD] + [BOS] + ids_of("abc") + [SEP] + ids_of("de") + [SEP]]
    assert types == [[0, 0, 0, 0, 0, 0, 1, 1, 1]] and (first_len, second_len) == ([3], [2])


def test_ties(tok):
    """equally long sides lose from the second first: odd C leaves the first one more"""
    for C, keep in ((3, (2, 1)), (4, (2, 2)), (1, (1, 0)), (9, (5, 4)), (10, (5, 5))):
        rows, types, _p, _s, first_len, second_len = tok.encode_batch_pairs(["abcde"], ["vwxyz"], C)
        assert (first_len, second_len) == ([keep[0]], [keep[1]]), C
        assert rows == [ids_of("abcde"[:keep[0]]) + ids_of("vwxyz"[:keep[1]])] and types == [[0] * keep[0] + [1] * keep[1]]
    # the longer side comes down to the shorter before the shorter loses anything
    assert tok.encode_batch_pairs(["abcdefgh"], ["xyz"], 7)[4:6] == ([4], [3])
    assert tok.encode_batch_pairs(["abc"], ["stuvwxyz"], 7)[4:6] == ([3], [4])
    assert tok.encode_batch_pairs(["abc"], ["stuvwxyz"], 5)[4:6] == ([3], [2])
    assert tok.encode_batch_pairs(["abcd"], ["stuvwxyz"], 5)[4:6] == ([3], [2])


def test_only_one_side(tok):
    first, second = "abcdef", "uvwxyz"
    for L, mode, keep in ((8, "only_first", (2, 6)), (8, "only_second", (6, 2)), (6, "only_first", (0, 6)), (4, "only_first", (0, 4)),
                          (4, "only_second", (4, 0)), (12, "only_first", (6, 6)), (13, "only_second", (6, 6))):
        rows, types, _p, _s, first_len, second_len = tok.encode_batch_pairs([first], [second], L, truncation=mode, pad_id=PAD)
        assert (first_len, second_len) == ([keep[0]], [keep[1]]), (L, mode)
        assert rows == [ids_of(first[:keep[0]]) + ids_of(second[:keep[1]]) + [PAD] * (L - sum(keep))]
        assert types == [[0] * keep[0] + [1] * keep[1] + [0] * (L - sum(keep))]


def test_windows_carry_the_whole_question(tok):
    q, ctx = "who", "0123456789"
    rows, types, row_pair, row_start, first_len, second_len, spans = tok.encode_batch_pairs(
        [q, ""], [ctx, ""], 10, truncation="windows", stride=1, sep_id=SEP, pad_id=PAD, bos_id=BOS, eos_id=EOS, offsets="char")
    # C = 7, ka = 3, Cb = 4, step = 3
    assert row_pair == [0, 0, 0, 1] and row_start == [0, 3, 6, 0] and first_len == [3, 3, 3, 0] and second_len == [4, 4, 4, 0]
    for r, s in enumerate((0, 3, 6)):
        assert rows[r] == [BOS] + ids_of(q) + [SEP] + ids_of(ctx[s:s + 4]) + [EOS] and types[r] == [0] * 5 + [1] * 5
        assert spans[r] == [(0, 0), (0, 1), (1, 2), (2, 3), (0, 0)] + [(s + k, s + k + 1) for k in range(4)] + [(0, 0)]
    assert rows[3] == [BOS, SEP, EOS] + [PAD] * 7 and types[3] == [0, 0, 1] + [0] * 7 and spans[3] == [(0, 0)] * 10
    # a long first side leaves stride + 1 slots for the second
    out = tok.encode_batch_pairs(["abcdefghij"], ["0123"], 6, truncation="windows", stride=2)
    assert out[4] == [3, 3] and out[3] == [0, 1] and out[5] == [3, 3] and out[0] == [ids_of("abc012"), ids_of("abc123")]


def test_spans_are_in_the_slots_own_text(tok):
    first, second = "the é", "中 then"
    for unit in ("char", "byte"):
        out = tok.encode_batch_pairs([first], [second], 16, sep_id=SEP, bos_id=BOS, eos_id=EOS, pad_id=PAD, padding_side="left", offsets=unit)
        (ia, sa), (ib, sb) = tok.encode_with_offsets(first, unit), tok.encode_with_offsets(second, unit)
        seq = [BOS] + ia + [SEP] + ib + [EOS]
        fill = 16 - len(seq)
        assert out[0] == [[PAD] * fill + seq]
        assert out[6] == [[(0, 0)] * (fill + 1) + sa + [(0, 0)] + sb + [(0, 0)]]
        assert out[1] == [[0] * (fill + 2 + len(ia)) + [1] * (len(ib) + 1)]


def test_an_empty_second_is_a_padded_batch(tok):
    for L, bos, eos, side in itertools.product((1, 2, 3, 7, 50), (None, BOS), (None, 0), ("right", "left")):
        n_added = (bos is not None) + (eos is not None)
        if L <= n_added:
            continue
        exp_rows, exp_len = tok.encode_batch_padded(HAND, L, pad_id=PAD, bos_id=bos, eos_id=eos, padding_side=side)
        for mode in ("longest_first", "only_first", "only_second"):
            rows, _types, row_pair, row_start, first_len, second_len = tok.encode_batch_pairs(
                HAND, [""] * len(HAND), L, truncation=mode, pad_id=PAD, bos_id=bos, eos_id=eos, padding_side=side)
            assert rows == exp_rows and [k + n_added for k in first_len] == exp_len, (L, bos, eos, side, mode)
            assert row_pair == list(range(len(HAND))) and not any(row_start) and not any(second_len)


def test_an_empty_first_is_a_windows_batch(tok):
    for L, bos, eos, side in itertools.product((1, 2, 3, 7, 50), (None, BOS), (None, 0), ("right", "left")):
        n_added = (bos is not None) + (eos is not None)
        for stride in sorted({0, 1, L - n_added - 1} & set(range(L - n_added))):
            for offsets in (None, "char", "byte"):
                kw = dict(pad_id=PAD, bos_id=bos, eos_id=eos, padding_side=side, offsets=offsets)
                exp = tok.encode_batch_windows(HAND, L, stride, **kw)
                got = tok.encode_batch_pairs([""] * len(HAND), HAND, L, truncation="windows", stride=stride, **kw)
                assert got[0] == exp[0] and got[2] == exp[1] and got[3] == exp[2], (L, stride, bos, eos, side)
                assert [k + n_added for k in got[5]] == exp[3] and not any(got[4])
                if offsets:
                    assert got[6] == exp[4]


def test_defaults(tok):
    with_pad = BBPETokenizer(vocab={**IDENT, b"[PAD]": 999}, merges=[])
    assert with_pad.encode_batch_pairs(["a"], ["b"], 3)[0] == [[97, 98, 999]]
    assert tok.encode_batch_pairs(["a"], ["b"], 3)[0] == [[97, 98, 0]]
    assert tok.encode_batch_pairs(["a"], ["b"], 3, sep_id=SEP)[0] == [[97, SEP, 98]]            # one separator by default
    assert tok.encode_batch_pairs(["a"], ["b"], 3, n_sep=2)[0] == [[97, 98, 0]]                 # n_sep counts only with a sep_id
    assert tok.encode_batch_pairs(["a"], ["b"], 3, sep_id=SEP, n_sep=0)[0] == [[97, 98, 0]]
    assert tok.encode_batch_pairs([], [], 3) == ([], [], [], [], [], [])
    assert tok.encode_batch_pairs([], [], 3, offsets="byte") == ([], [], [], [], [], [], [])
    assert tok.encode_batch_pairs(("a",), iter(["b"]), 2)[0] == [[97, 98]]                      # any sequences of str


def test_value_errors(tok):
    good = dict(firsts=["a", "b"], seconds=["c", "d"], max_length=8)
    bad = [
        dict(seconds=["c"]),                                       # unequal lengths
        dict(firsts="ab"), dict(seconds="cd"), dict(firsts=[b"a", b"b"]), dict(seconds=["c", 5]), dict(firsts=None), dict(seconds=7),
        dict(truncation="longest"), dict(truncation="left"), dict(truncation=None), dict(truncation=True),
        dict(stride=1), dict(stride=-1), dict(truncation="only_first", stride=2), dict(truncation="only_second", stride=1),
        dict(truncation="windows", stride=8), dict(truncation="windows", stride=-1), dict(truncation="windows", stride=1.5),
        dict(truncation="windows", stride=5, bos_id=1, eos_id=2, sep_id=3),   # C = 5: stride at most 4
        dict(sep_id=1, n_sep=3), dict(n_sep=3), dict(n_sep=-1), dict(sep_id=1, n_sep=None), dict(n_sep=True),
        dict(max_length=0), dict(max_length=1, bos_id=1), dict(max_length=2, bos_id=1, eos_id=2), dict(max_length=3, bos_id=1, eos_id=2, sep_id=3),
        dict(max_length=4, bos_id=1, eos_id=2, sep_id=3, n_sep=2), dict(max_length=None), dict(max_length=2.5),
        dict(pad_id=-1), dict(bos_id=1 << 32), dict(eos_id="x"), dict(sep_id=-1), dict(sep_id=1 << 32), dict(sep_id=2.0), dict(pad_id=1.0),
        dict(padding_side="top"), dict(offsets="word"),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            tok.encode_batch_pairs(**{**good, **kw})
    # the edges that are fine
    assert len(tok.encode_batch_pairs(**good, truncation="windows", stride=7)[0]) == 2
    assert tok.encode_batch_pairs(["a"], ["b"], 5, bos_id=1, eos_id=2, sep_id=3, n_sep=2)[0] == [[1, 97, 3, 3, 2]]
    assert tok.encode_batch_pairs(["a"], ["b"], 2, sep_id=(1 << 32) - 1)[0] == [[97, (1 << 32) - 1]]
