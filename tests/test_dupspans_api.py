"""CPU: the plain-Python exact-substring rule (BBPETokenizer.duplicate_spans / remove_duplicate_spans / encode_batch_dedup) --
what the kernels of csrc/yabpe_dup_kernels.h are held to -- against the brute force of dup_helpers.py."""
from __future__ import annotations

import pytest

from tests import dup_helpers as dh, mask_helpers
from yet_another_bpe.tokenizer import BBPETokenizer

TOK = BBPETokenizer()


@pytest.mark.parametrize("n", dh.MIN_LENS)
@pytest.mark.parametrize("name", dh.CORPORA)
def test_rule_equals_brute_force(name, n):
    docs = dh.corpus(name, n)
    masks, n_dup, n_windows, n_repeats = dh.brute(name, n)
    got, got_n, st = TOK.duplicate_spans(docs, min_len=n)
    assert got == masks and got_n == n_dup
    spans = sum(m[j] and not (j and m[j - 1]) for m in masks for j in range(len(m)))
    assert st == {"n_ids": sum(map(len, docs)), "n_docs": len(docs), "n_windows": n_windows, "n_repeats": n_repeats, "n_dup_ids": sum(n_dup),
                  "n_spans": spans, "n_kept": sum(map(len, docs)) - sum(n_dup)}
    kept, kept_n = TOK.remove_duplicate_spans(docs, min_len=n)
    assert kept_n == n_dup and kept == [[t for t, m in zip(d, mk) if not m] for d, mk in zip(docs, masks)]
    assert n_repeats > 0


def test_hand_cases():
    # a run of one id of length L keeps n and loses L - n
    assert TOK.duplicate_spans([[4] * 7], min_len=3)[0] == [[0, 0, 0, 1, 1, 1, 1]]
    # an overlapping equal window is no repeat: abab|ab -> the window at 2 overlaps the one at 0, the one at 4 does not
    assert TOK.duplicate_spans([[1, 2] * 4], min_len=4)[0] == [[0, 0, 0, 0, 1, 1, 1, 1]]
    # windows never cross a seam; the first occurrence stays, wherever its document stands
    masks, n_dup, st = TOK.duplicate_spans([[1, 2], [3, 1, 2, 3], [], [2, 3, 1]], min_len=3)
    assert masks == [[0, 0], [0, 0, 0, 0], [], [0, 0, 0]] and st["n_windows"] == 3
    assert TOK.remove_duplicate_spans([[1, 2, 3], [9, 1, 2, 3], [1, 2, 3]], min_len=3) == ([[1, 2, 3], [9], []], [0, 3, 3])
    assert TOK.duplicate_spans([], min_len=1)[2]["n_docs"] == 0


@pytest.mark.parametrize("bad", [0, -1, 1025, 2.5, None, "5"])
def test_min_len_out_of_range_is_refused(bad):
    for call in (lambda: TOK.duplicate_spans([[1]], min_len=bad), lambda: TOK.remove_duplicate_spans([[1]], min_len=bad),
                 lambda: TOK.encode_batch_dedup(["a"], bad), lambda: TOK.duplicate_spans_array([1], [0, 1], min_len=bad),
                 lambda: TOK.encode_array_dedup(["a"], bad)):  # (refused before a device is looked for)
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("off", [[1, 2], [0, 1], [0, 3, 2], [[0, 2]], []])
def test_offsets_that_do_not_fit_are_refused(off):
    with pytest.raises(ValueError):
        TOK.duplicate_spans_array([5, 6], off)


def test_repeated_paragraphs_leave_the_text():
    tok = mask_helpers.tokenizer()
    words = mask_helpers.corpus_words()
    para = " " + " ".join(words[100:160])
    texts = ["intro" + para + " tail one", "", "other" + para + " tail two" + para]
    ids, n_dup = tok.encode_batch_dedup(texts, min_len=20)
    assert n_dup[0] == 0 and n_dup[2] > 2 * 40 and [tok.decode(x) for x in ids][0] == texts[0]
    assert " ".join(words[110:150]) not in tok.decode(ids[2]) and tok.decode(ids[2]).startswith("other")
