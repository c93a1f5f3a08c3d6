"""CPU: the inputs of tests/test_gpu_exchange.py force the branches those tests are about -- with buffers of 4 records the
corpus.en job must reallocate its exchange buffers at least three times (so areas of 4, 16 and 64 records are each outgrown),
one of its exchanges carries no record at all, and the shapes corpus really leaves rank 0 with long words only, rank 1 with
nothing and rank 3 with one tile, while the oracle still finds every merge asked for."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

from oracle import oracle
from tests import exchange_workers as xw, helpers

MERGES = 300


def changed_pairs(words, merges, world):
    """The oracle's merges replayed on every rank's shard (plan_shards): [merge][rank] = the distinct pairs whose count on that
    rank changes with the merge, the merged pair left out -- each of them is at least one record of that rank's exchange."""
    from yet_another_bpe.distributed import plan_shards

    _flat, off = helpers.flatten(words)
    shards = []
    for w0, w1 in plan_shards(off, world):
        pool = Counter(words[w0:w1])  # (equal words change alike: one replay per distinct word)
        shards.append([[tuple(bytes([b]) for b in w), f] for w, f in pool.items()])
    out = []
    for x, y in merges:
        z = x + y
        row = []
        for shard in shards:
            delta = Counter()
            for entry in shard:
                w, f = entry
                if not any(w[j] == x and w[j + 1] == y for j in range(len(w) - 1)):
                    continue
                new, j = [], 0
                while j < len(w):
                    if j + 1 < len(w) and w[j] == x and w[j + 1] == y:
                        new.append(z)
                        j += 2
                    else:
                        new.append(w[j])
                        j += 1
                for j in range(len(w) - 1):
                    delta[(w[j], w[j + 1])] -= f
                for j in range(len(new) - 1):
                    delta[(new[j], new[j + 1])] += f
                entry[0] = tuple(new)
            row.append(sum(1 for k, v in delta.items() if v != 0 and k != (x, y)))
        out.append(row)
    return out


@pytest.fixture(scope="module")
def corpus():
    words = helpers.corpus_en_words()
    assert len(words) == 28772
    merges = oracle.merge_loop(words, 257 + MERGES, 1, xw.SP)[1]
    assert len(merges) == MERGES
    return words, merges


@pytest.mark.parametrize("world,largest,above_64,above_16", [(2, 117, 34, 183), (4, 101, 25, 162)])
def test_buffers_of_4_records_are_outgrown_three_times(corpus, world, largest, above_64, above_16):
    """From delta_cap = 4 the buffers grow fourfold per reallocation: a rank with more than 64 records to send needs 256."""
    words, merges = corpus
    per_merge = [max(row) for row in changed_pairs(words, merges, world)]
    print(f"world {world}: largest {max(per_merge)} at merge {per_merge.index(max(per_merge))}, above 64: {sum(n > 64 for n in per_merge)}, "
          f"above 16: {sum(n > 16 for n in per_merge)}, above 4: {sum(n > 4 for n in per_merge)}")
    assert max(per_merge) == largest and per_merge.index(largest) == 29
    assert sum(n > 64 for n in per_merge) == above_64
    assert sum(n > 16 for n in per_merge) == above_16
    assert 64 < largest <= 256  # 4 -> 16 -> 64 -> 256: three reallocations at least, and areas of 4, 16 and 64 records are outgrown


@pytest.mark.parametrize("world", [2, 4])
def test_one_exchange_is_empty(corpus, world):
    words, merges = corpus
    assert changed_pairs(words, merges[:8], world)[7] == [0] * world


def test_the_reversed_corpus_has_200_merges(corpus):
    words, _merges = corpus
    assert len(oracle.merge_loop(words[::-1], 257 + 200, 1, xw.SP)[1]) == 200


def test_shapes():
    short_all = helpers.corpus_en_words()
    words, freq, ranges = xw.shapes_corpus("flat")
    assert freq is None and len(ranges) == 4
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = ranges
    assert a0 == 0 and a1 == b0 == b1 == c0 and c1 == d0 and d1 == len(words)
    assert words[a0:a1] == [b" " * 900, b"ab" * 700, b"xyz" * 50] * 3 and all(len(w) > 63 for w in words[a0:a1])
    assert 1900 <= c1 - c0 <= 2100 and words[c0:c1] == short_all[xw.SHORT_SLICE[0]:xw.SHORT_SLICE[1]]
    assert all(0 < len(w) <= 63 for w in words[c0:c1])
    assert d1 - d0 == 1 and len(words[d0]) == 2 and words[d0] not in words[c0:c1]
    # world 2: long words only | everything else
    words2, _freq, ranges2 = xw.shapes_corpus("flat", 2)
    assert words2 == words and ranges2 == [(0, a1), (a1, len(words))]
    # the weighted layout: the same words pooled, the same four shapes
    uw, fq, wr = xw.shapes_corpus("weighted")
    assert dict(zip(uw, fq.tolist())) == dict(Counter(words)) and len(set(uw)) == len(uw) and fq.dtype == np.uint64
    (a0, a1), (b0, b1), (c0, c1), (d0, d1) = wr
    assert a0 == 0 and a1 == b0 == b1 == c0 == 3 and c1 == d0 and d1 == len(uw)
    assert uw[:3] == [b" " * 900, b"ab" * 700, b"xyz" * 50] and fq[:3].tolist() == [3, 3, 3]
    assert c1 - c0 > 500 and all(0 < len(w) <= 63 for w in uw[c0:c1]) and int(fq[c0:c1].max()) > 1
    assert uw[d0] == xw.LONE_WORD and int(fq[d0]) == 1
    assert xw.shapes_corpus("weighted", 2)[2] == [(0, 3), (3, len(uw))]
    # the oracle finds every merge asked for, in both layouts (and they are the same merges: pooling changes no count)
    flat_merges = oracle.merge_loop(words, 257 + xw.SHAPES_MERGES, 1, xw.SP)[1]
    weighted_merges = oracle.train_flat(*helpers.flatten(uw), 257 + xw.SHAPES_MERGES, 1, xw.SP, freq=fq)[1]
    assert len(flat_merges) == xw.SHAPES_MERGES and len(weighted_merges) == xw.SHAPES_MERGES
    assert flat_merges == weighted_merges
    # the long words take part: merges of their pairs are among the first
    assert (b" ", b" ") in flat_merges[:10] and (b"a", b"b") in flat_merges[:10]
