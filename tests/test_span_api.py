"""CPU: the plain-Python span corruption of BBPETokenizer -- span_thresholds, corrupt_spans, encode_batch_span_corrupted:
an example worked by hand from printed draws, the T5 shape, sentinels by string, every refused argument, first_doc (a shard
equals the slice of the whole batch), and a result that depends neither on the surrounding batch nor on the row lengths."""
from __future__ import annotations

import pytest

from tests import mask_helpers as mh
from yet_another_bpe.synth import rnd_int
from yet_another_bpe.tokenizer import BBPETokenizer

S = [900, 901, 902, 903]


def test_thresholds():
    To, C = BBPETokenizer.span_thresholds(0.15, 3.0, 10)
    assert To == 232811675 and len(C) == 9
    assert C[0] == int((1 - 1 / 3.0) * 2**32) and all(a >= b for a, b in zip(C, C[1:])) and C[-1] > 0
    assert BBPETokenizer.span_thresholds(0.15, 3.0, 1) == (BBPETokenizer._dropout_threshold(0.15), [])  # Lmax 1: To = T(p)
    assert BBPETokenizer.span_thresholds(0, 3.0, 10)[0] == 0
    assert BBPETokenizer.span_thresholds(1, 3.0, 10)[0] >= 2**32 - 1
    assert BBPETokenizer.span_thresholds(0.5, 1.0, 4) == (BBPETokenizer.span_thresholds(0.5, 1.0, 1)[0], [0, 0, 0])  # mean 1: every span one unit
    assert len(BBPETokenizer.span_thresholds(0.5, 5, 32)[1]) == 31
    a, b = BBPETokenizer.span_thresholds(0.15, 3.0, 10)[0], BBPETokenizer.span_thresholds(0.3, 3.0, 10)[0]
    assert a < b < 2 * a * 1.2  # more noise, more openers


def test_an_example_worked_by_hand():
    """p = 0.3, mean 3, Lmax 4, seed 1: To = 603318222, C = [2863311530, 1908874353, 1272582902].  The draws r = rnd(Kd, 0x6f, u)
    as (r >> 32, r & 0xFFFFFFFF), printed from synth.rnd_int, of the units that open (r >> 32 < To):
      document 0 (Kd = rnd(1, 0x63, 0)):  u = 6: (228396800, 639147699) -- x below all of C: length 4, covers 6 .. 9;
                                          u = 9: (267675874, 2494928032) -- x below C[0] alone: length 2, covers 9, 10.
      document 1 (Kd = rnd(1, 0x63, 1)):  u = 0: (306551024, 3446663036) -- x above C[0]: length 1;
                                          u = 3: (387824769, 1213544690) -- length 4, covers 3 .. 6: the document ends at 5;
                                          u = 5: (596550139, 821793713) -- length 4.
    So document 0 (12 tokens) has one run, tokens 6 .. 10 (two spans merged), and document 1 (6 tokens) the runs {0}, {3, 4, 5}."""
    To, C = BBPETokenizer.span_thresholds(0.3, 3.0, 4)
    assert (To, C) == (603318222, [2863311530, 1908874353, 1272582902])
    opens = {d: [u for u in range(12) if rnd_int(rnd_int(1, 0x63, d), 0x6f, u) >> 32 < To] for d in (0, 1)}
    assert opens == {0: [6, 9], 1: [0, 3, 5]}
    assert rnd_int(rnd_int(1, 0x63, 0), 0x6f, 6) == (228396800 << 32) | 639147699
    tok = BBPETokenizer()
    docs = [list(range(10, 22)), list(range(30, 36))]
    kw = {"sentinels": S, "p": 0.3, "mean_span_length": 3.0, "max_span_length": 4, "seed": 1}
    inputs, targets = tok.corrupt_spans(docs, **kw)
    assert inputs == [[10, 11, 12, 13, 14, 15, 900, 21], [900, 31, 32, 901]]
    assert targets == [[900, 16, 17, 18, 19, 20, 901], [900, 30, 901, 33, 34, 35, 902]]
    inputs, targets = tok.corrupt_spans(docs, final_sentinel=False, **kw)
    assert inputs == [[10, 11, 12, 13, 14, 15, 900, 21], [900, 31, 32, 901]] and targets == [[900, 16, 17, 18, 19, 20], [900, 30, 901, 33, 34, 35]]
    # the cut: inside document 0's run, and on the start of document 1's second run
    inputs, targets = tok.corrupt_spans(docs, max_tokens=8, **kw)
    assert inputs == [[10, 11, 12, 13, 14, 15, 900], [900, 31, 32, 901]] and targets == [[900, 16, 17, 901], [900, 30, 901, 33, 34, 35, 902]]
    inputs, targets = tok.corrupt_spans(docs, max_tokens=3, **kw)
    assert inputs == [[10, 11, 12], [900, 31, 32]] and targets == [[900], [900, 30, 901]]
    # the sentinel cap: two sentinels, one of them the final one -- document 1's second run stays in the input
    inputs, targets = tok.corrupt_spans(docs, **{**kw, "sentinels": S[:2]})
    assert inputs == [[10, 11, 12, 13, 14, 15, 900, 21], [900, 31, 32, 33, 34, 35]] and targets == [[900, 16, 17, 18, 19, 20, 901], [900, 30, 901]]
    inputs, targets = tok.corrupt_spans(docs, final_sentinel=False, **{**kw, "sentinels": S[:1]})
    assert inputs[1] == [900, 31, 32, 33, 34, 35] and targets == [[900, 16, 17, 18, 19, 20], [900, 30]]
    # a special inside the run of document 0 splits it: two runs, two sentinels; whole words: units from the words
    special = [[j == 8 for j in range(12)], [False] * 6]
    inputs, targets = tok.corrupt_spans(docs, None, special, **kw)
    assert inputs[0] == [10, 11, 12, 13, 14, 15, 900, 18, 901, 21] and targets[0] == [900, 16, 17, 901, 19, 20, 902]
    words = [[0, 0, 1, 2, 3, 3, 3, 4, 5, 5, 5, 5], [0, 0, 0, 1, 2, 2]]  # document 0: no token of the units 6 .. 10: nothing is noise
    inputs, targets = tok.corrupt_spans(docs, words, None, whole_word=True, **kw)
    assert inputs == [docs[0], [900, 33, 34, 35]] and targets == [[900], [900, 30, 31, 32, 901]]
    words = [[0, 1, 2, 3, 4, 5, 5, 6, 6, 6, 7, 11], [0] * 6]  # unit 6 opens (6 .. 9), unit 9 has no token, unit 11 is free
    inputs, targets = tok.corrupt_spans(docs, words, None, whole_word=True, **kw)
    assert inputs[0] == [10, 11, 12, 13, 14, 15, 16, 900, 21] and targets[0] == [900, 17, 18, 19, 20, 901]


def test_the_t5_shape():
    tok = mh.tokenizer()
    text = "Thank you for inviting me to your party last week and for the cake"
    ids = tok.encode(text)
    sent = ["[MASK]", "[PAD]", "<|endoftext|>"]
    s = [tok._vocab[x.encode()] for x in sent]
    for seed in range(200):  # the first seed with exactly two runs, none at either end: A <s0> B <s1> C and <s0> x.. <s1> z.. <s2>
        (row,), (tgt,) = tok.corrupt_spans([ids], sentinels=sent, p=0.3, seed=seed)
        if [x for x in row if x in s] == s[:2] and row[0] not in s and row[-1] not in s:
            break
    else:
        raise AssertionError("no seed gives two inner runs")
    i0, i1 = row.index(s[0]), row.index(s[1])
    A, B, C = row[:i0], row[i0 + 1:i1], row[i1 + 1:]
    assert tgt[0] == s[0] and tgt[-1] == s[2] and tgt.count(s[1]) == 1
    t1 = tgt.index(s[1])
    x, z = tgt[1:t1], tgt[t1 + 1:-1]
    assert x and z and A and B and C and A + x + B + z + C == ids
    assert tok.decode(A + x + B + z + C) == text


def test_sentinels_by_string():
    tok = mh.tokenizer()
    ids = [tok.encode(t) for t in ("one two three four five six seven eight nine ten", "", "eleven")]
    by_name = tok.corrupt_spans(ids, sentinels=["[MASK]", "[PAD]", "<|endoftext|>"], p=0.4, seed=3)
    by_id = tok.corrupt_spans(ids, sentinels=[tok._vocab[b"[MASK]"], tok._vocab[b"[PAD]"], tok._vocab[b"<|endoftext|>"]], p=0.4, seed=3)
    assert by_name == by_id and by_name[0][1] == by_name[1][1] == []
    mixed = tok.corrupt_spans(ids, sentinels=["[MASK]", 70000, "<|endoftext|>"], p=0.4, seed=3)
    assert mixed != by_id and [[70000 if x == tok._vocab[b"[PAD]"] else x for x in r] for r in by_id[1]] == mixed[1]
    for bad in (["nope"], [mh.NO_ID, "[MASK]"], ["one", "[MASK]"], "[MASK]", None, [-1, 2], [1 << 32, 2], [1.5, 2]):
        with pytest.raises(ValueError):  # not a special; a special without an id; a word of the vocab; no sequence; no u32
            tok.corrupt_spans(ids, sentinels=bad)


def test_refused_arguments():
    tok = BBPETokenizer()
    docs = [[1, 2, 3]]
    assert tok.corrupt_spans(docs, sentinels=S, p=0) == ([[1, 2, 3]], [[900]])
    for bad in ({"p": -0.1}, {"p": 1.5}, {"p": float("nan")}, {"p": "0.1"}, {"mean_span_length": 0.5}, {"mean_span_length": float("inf")},
                {"mean_span_length": None}, {"max_span_length": 0}, {"max_span_length": 33}, {"max_span_length": 2.5}, {"sentinels": []},
                {"sentinels": [900]}, {"whole_word": True}, {"max_tokens": 0}, {"max_tokens": -3}, {"max_tokens": 1.5}, {"seed": -1}, {"seed": 1 << 64},
                {"first_doc": 1 << 64}):
        with pytest.raises(ValueError):
            tok.corrupt_spans(docs, **{"sentinels": S, **bad})
    assert tok.corrupt_spans(docs, sentinels=[900], final_sentinel=False, p=0) == ([[1, 2, 3]], [[]])
    assert tok.corrupt_spans([], sentinels=S) == ([], [])
    mt = mh.tokenizer()
    for bad in ({"max_length": -1}, {"max_target_length": -1}, {"max_length": 1, "bos_id": 5, "eos_id": 6}, {"max_target_length": 1, "bos_id": 5, "eos_id": 6},
                {"truncation": "middle"}, {"padding_side": "up"}, {"sentinels": []}, {"p": 2}):
        with pytest.raises(ValueError):
            mt.encode_batch_span_corrupted(["a b c"], **{"sentinels": ["[MASK]", "[PAD]"], **bad})


def test_first_doc_a_shard_equals_the_slice_of_the_batch():
    tok = BBPETokenizer()
    ids_b, words_b, special_b = mh.synth_batch([30, 0, 7, 120, 1, 64], seed=4)
    for whole_word in (False, True):
        kw = {"sentinels": list(range(9000, 9050)), "p": 0.4, "seed": 11, "whole_word": whole_word}
        whole = tok.corrupt_spans(ids_b, words_b, special_b, first_doc=100, **kw)
        for a, b in ((0, 2), (2, 6), (3, 4)):
            part = tok.corrupt_spans(ids_b[a:b], words_b[a:b], special_b[a:b], first_doc=100 + a, **kw)
            assert part == (whole[0][a:b], whole[1][a:b])
        assert tok.corrupt_spans(ids_b, words_b, special_b, first_doc=101, **kw) != whole
        assert tok.corrupt_spans(ids_b, words_b, special_b, first_doc=100, **{**kw, "seed": 12}) != whole
    # the span draws are not the mask draws of the same seed: a document key of their own
    assert rnd_int(11, 0x63, 100) != rnd_int(11, 0x6d, 100)


def test_the_result_depends_neither_on_the_batch_nor_on_the_row_lengths():
    tok = mh.tokenizer()
    texts = ["The quick brown fox jumps over the lazy dog again and again.", "", "<|endoftext|>Hello there[MASK] world", "x " * 40]
    kw = {"sentinels": ["[MASK]", "[PAD]"] + list(range(5000, 5030)), "p": 0.4, "seed": 5}
    rows, labels, lengths, label_lengths = tok.encode_batch_span_corrupted(texts, **kw)
    enc = tok.encode_batch_with_words(texts)
    inputs, targets = tok.corrupt_spans([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], **kw)
    assert [r[:n] for r, n in zip(rows, lengths)] == inputs and [r[:n] for r, n in zip(labels, label_lengths)] == targets
    assert all(set(r[n:]) <= {tok._vocab[b"[PAD]"]} for r, n in zip(rows, lengths)) and all(set(r[n:]) <= {-100} for r, n in zip(labels, label_lengths))
    assert len({len(r) for r in rows}) == 1 and len(rows[0]) == max(lengths) and len(labels[0]) == max(label_lengths)
    # specials are never removed
    eot = tok._vocab[b"<|endoftext|>"]
    assert inputs[2][0] == eot and tok._vocab[b"[MASK]"] in inputs[2]
    # other row lengths cut the same sequences; BOS and EOS frame them, -100 in their label slots
    r8, l8, n8, m8 = tok.encode_batch_span_corrupted(texts, 8, 5, **kw)
    assert [r[:n] for r, n in zip(r8, n8)] == [x[:8] for x in inputs] and [r[:n] for r, n in zip(l8, m8)] == [x[:5] for x in targets]
    rb, lb, nb, mb = tok.encode_batch_span_corrupted(texts, 8, 5, bos_id=7001, eos_id=7002, **kw)
    assert rb[0] == [7001] + inputs[0][:6] + [7002] and lb[0] == [-100] + targets[0][:3] + [-100] and (nb[1], mb[1]) == (2, 2)
    # alone or in another batch (with first_doc): the same rows
    alone = tok.encode_batch_span_corrupted(texts[3:], first_doc=3, **kw)
    assert alone[0][0][:alone[2][0]] == inputs[3] and alone[1][0][:alone[3][0]] == targets[3]
    # max_tokens cuts the documents before the layout; the draws are the same
    cut_in, cut_tgt = tok.corrupt_spans([e[0] for e in enc], [e[1] for e in enc], [e[2] for e in enc], max_tokens=6, **kw)
    r6 = tok.encode_batch_span_corrupted(texts, max_tokens=6, **kw)
    assert [r[:n] for r, n in zip(r6[0], r6[2])] == cut_in and [r[:n] for r, n in zip(r6[1], r6[3])] == cut_tgt
