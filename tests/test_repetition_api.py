"""CPU: BBPETokenizer.repetition_stats on cases whose signals are written out by hand, and repetition_keep at its bounds."""
from __future__ import annotations

import pytest

from yet_another_bpe.tokenizer import BBPETokenizer

TOK = BBPETokenizer()


@pytest.mark.parametrize("ids, n, expected", [
    ([7] * 6, 2, (5, 1, 6)),                  # one class of five overlapping windows
    ([1, 2, 3, 1, 2, 3, 1], 3, (2, 3, 7)),    # (1,2,3) and (2,3,1) twice, (3,1,2) once: every id inside a repeated window
    ([1, 2, 3, 4], 2, (1, 3, 0)),             # nothing repeats
    ([1, 2, 3], 4, (0, 0, 0)),                # L < n: no window
    ([5, 6, 9, 5, 6, 8, 8], 1, (2, 4, 6)),    # n = 1: unique ids; 9 is the one id that occurs once
    ([5, 6, 9, 5, 6, 8, 8], 2, (2, 5, 4)),    # (5,6) twice: positions 0, 1, 3, 4
])
def test_signals_by_hand(ids, n, expected):
    top, distinct, covered = TOK.repetition_stats([ids, [], ids], ngrams=(n,))  # (the same document twice: they never meet)
    assert (top[0][0], distinct[0][0], covered[0][0]) == expected == (top[2][0], distinct[2][0], covered[2][0])
    assert (top[1], distinct[1], covered[1]) == ([0], [0], [0])


@pytest.mark.parametrize("ngrams", [(), tuple(range(1, 18)), (0,), (65,), (2, 2), (3, 2), (2.5,)])
def test_lengths_are_checked(ngrams):
    with pytest.raises(ValueError):
        TOK.repetition_stats([[1, 2]], ngrams=ngrams)


def test_keep_at_the_bounds():
    ngrams = (2, 5, 11)  # (11: in neither table -- skipped whatever it holds)
    lengths = [100, 100, 100, 100, 0, 100, 100]
    top = [[10, 1, 99], [11, 1, 0], [1, 1, 0], [2, 1, 0], [0, 0, 0], [1, 1, 0], [1, 1, 0]]
    covered = [[0, 0, 99], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [100, 15, 0], [100, 16, 0]]
    keep = BBPETokenizer.repetition_keep(lengths, top, covered, ngrams)
    # 10 * 2 / 100 = .20 is not over the bound, 11 * 2 / 100 is; top == 1 fails nothing; the empty document stays;
    # covered 15 / 100 = .15 is not over the bound of n = 5, 16 / 100 is (covered at n = 2 is in no table)
    assert keep.tolist() == [True, False, True, True, True, True, False]
    assert BBPETokenizer.repetition_keep([4], [[4]], [[4]], (2,), top_max={2: 2.0}).tolist() == [True]
    assert BBPETokenizer.repetition_keep([4], [[1]], [[0]], (2,), top_max={2: 0.1}).tolist() == [True]  # top == 1: 1 * 2 / 4 > .1, but nothing repeats
    assert BBPETokenizer.repetition_keep([4], [[2]], [[0]], (2,), top_max={2: 0.1}).tolist() == [False]
