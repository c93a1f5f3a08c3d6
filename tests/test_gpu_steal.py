"""GPU (-m gpu): the sparse launch's second round.  A stream of more chunks than scan workgroups (forced here with
full_skip_blocks on a few MiB; in production the early sparse merges of a large corpus) hands the tiles behind the first
round out in pieces, from one tagged counter, to whichever workgroup finishes first (option chunk_steal, 1 by default; 0 =
dealt by workgroup index).  Who rewrites a tile must not matter: merges, vocabulary ids and pair counts are compared
bit-exactly with the C oracle, nothing left out, for both settings, both layouts, 8- and 16-wave workgroups (the 16-wave
form has no counter path and deals by index), one merge per launch and batches of up to 16.

The corpora hold, all through the stream, words that are exactly one pair (the word leaves the stream), runs of one letter
(a == b) and alternating letters (touching sites: the general rewrite).  The skewed one keeps every occurrence of the pairs
of the first few hundred merges in the first eighth of the words: the first workgroup's chunk holds the candidates, the
pieces of the second round hold none."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests import helpers

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]
N_MERGES = 160
CHUNK_MAX = 2048  # tiles a workgroup sweeps at a time at most (both workgroup widths)


def _corpus(seed: int, skewed: bool):
    rng = np.random.default_rng(seed)
    n_words = 1_150_000
    lens = rng.integers(2, 13, size=n_words)
    kind = rng.random(n_words)
    lens[kind < 0.04] = 2                      # exactly (a b)
    off = np.zeros(n_words + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    word_of = np.repeat(np.arange(n_words), lens)
    pos = np.arange(total) - np.repeat(off[:-1].astype(np.int64), lens)
    hot = np.frombuffer(b"etao", dtype=np.uint8)
    if skewed:
        cold = np.arange(48, 248, dtype=np.uint8)  # 200 values: a pair of them counts ~150, a hot pair ~50,000
        flat = cold[rng.integers(0, len(cold), size=total)]
        in_hot = word_of < n_words // 8
        flat[in_hot] = hot[rng.integers(0, 4, size=int(in_hot.sum()))]
        special = in_hot
    else:
        letters = np.frombuffer(b"etaoinshrdlu", dtype=np.uint8)
        p = np.array([12, 9, 8, 8, 7, 7, 6, 6, 6, 4, 4, 3], dtype=np.float64)
        flat = letters[rng.choice(len(letters), size=total, p=p / p.sum())]
        special = np.ones(total, dtype=bool)
    k = kind[word_of]
    runs = special & (k >= 0.04) & (k < 0.08)      # aaaa...
    flat[runs] = ord("e")
    alt = special & (k >= 0.08) & (k < 0.12)       # abab...
    flat[alt] = np.where(pos[alt] % 2 == 0, ord("t"), ord("a")).astype(np.uint8)
    two = special & (k < 0.04)                      # the word IS the pair
    flat[two] = np.where(pos[two] == 0, ord("t"), ord("a")).astype(np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


@pytest.fixture(scope="module", params=["skewed", "uniform"])
def case(request):
    flat, off = _corpus(17 if request.param == "skewed" else 23, request.param == "skewed")
    rng = np.random.default_rng(3)
    freq = rng.integers(1, 4, size=len(off) - 1).astype(np.uint64)
    base = helpers.base_tokens(SP)
    exp = {"flat": oracle.train_flat(flat, off, len(base) + N_MERGES, 1, SP, return_ids=True),
           "weights": oracle.train_flat(flat, off, len(base) + N_MERGES, 1, SP, return_ids=True, freq=freq)}
    return {"name": request.param, "flat": flat, "off": off, "freq": freq, "base": base, "exp": exp}


def _train(case, layout, options):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for k, v in {"verify": 1, "split": 1, **options}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(case["base"])
        ctx.load_words(case["flat"], case["off"], case["freq"] if layout == "weights" else None)
        tiles_loaded = ctx.stats()["n_tiles"]
        left, right, merged, count = ctx.train(N_MERGES, 1)
        st = ctx.stats()
        st["tiles_loaded"] = tiles_loaded  # (a retile shortens the stream later on)
        return left, right, merged, count, st


def _check(case, layout, options):
    left, right, merged, count, st = _train(case, layout, options)
    _vocab, _merges, ids = case["exp"][layout]
    what = (case["name"], layout, options)
    assert len(left) == N_MERGES == len(ids["left"]), what
    assert np.array_equal(left, ids["left"]) and np.array_equal(right, ids["right"]) and np.array_equal(merged, ids["merged"]), what
    assert np.array_equal(np.asarray(count, dtype=np.uint64), ids["count"]), what
    assert st["scan_skip_launches"] > 0, what
    return st


@pytest.mark.parametrize("layout", ["flat", "weights"])
@pytest.mark.parametrize("wpb", [8, 16])
@pytest.mark.parametrize("batch_max", [1, 16])
def test_second_round_equals_the_oracle(case, layout, wpb, batch_max):
    blocks = 3
    on = _check(case, layout, {"full_skip_blocks": blocks, "full_wpb": wpb, "batch_max": batch_max, "chunk_steal": 1})
    off = _check(case, layout, {"full_skip_blocks": blocks, "full_wpb": wpb, "batch_max": batch_max, "chunk_steal": 0})
    assert on["tiles_loaded"] > blocks * CHUNK_MAX, "the stream must be longer than one round of chunks"
    assert off["scan_skip_pieces_taken"] == 0
    if wpb == 8:
        assert on["scan_skip_pieces_taken"] > 0
    else:
        assert on["scan_skip_pieces_taken"] == 0  # (the 16-wave form deals by index)
    assert on["scan_skip_tiles_read"] == off["scan_skip_tiles_read"]  # the same tiles pass the signature test, whoever reads them


@pytest.mark.parametrize("blocks", [1, 2, 4])
def test_one_to_four_workgroups(case, blocks):
    """One workgroup takes every piece itself (pieces as large as a chunk); two and four race for a few small ones."""
    st = _check(case, "flat", {"full_skip_blocks": blocks, "full_wpb": 8})
    assert st["tiles_loaded"] > blocks * CHUNK_MAX
    assert st["scan_skip_pieces_taken"] > 0


def test_one_round_takes_nothing_from_the_counter(case):
    """The production geometry on a stream this short: every workgroup has one chunk, the counter is never touched."""
    st = _check(case, "flat", {})
    assert st["scan_skip_pieces_taken"] == 0
