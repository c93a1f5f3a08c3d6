"""GPU (-m gpu): the candidate-tile path of the sparse launch (k_scan_skip) reads the stream's buffers -- tiles, lengths,
signatures, and in the weighted layout the word bases and frequencies -- from the kernel's argument segment where it uses
them (SlowCtx's accessors over kernarg_read, csrc/yabpe_kernels.h) instead of carrying the pointers through its loop.  A wrong
offset, or an address rebuilt wrongly in a second round of chunks, writes a tile or a signature word to the wrong place: every
case runs the public training call with the sparse form forced from the first merge (split = 1), in the flat and the weighted
layout, with 8- and 16-wave workgroups (all four instantiations), is compared bit for bit with the C oracle (ids and counts of
every merge) and runs under verify = 1, where the incremental pair table must equal a recount of the stream at the end.

Shapes: ~64 KiB of words over a five-letter alphabet (heavy ties, batches above one merge; again with batch_max = 1); a
stream of exactly one tile; ~5,800 tiles swept by two scan workgroups of at most 2,048 tiles each (full_skip_blocks = 2: the
tiles behind the first round go out in a second one, dealt by index or -- 8-wave form, chunk_steal = 1 -- taken in pieces
from the counter, which the case asserts); and hand-made one-tile streams in which the only site of a pair stands at slot 0, at
510 / 511 / 512 (the seam between the two 512-slot segments), in the last live slots, and as a word that is exactly the pair
(the word leaves the stream: three slots) at the tile's start and across the seam.  A word of one letter takes two slots
(letter, separator): the filler that puts the site where the case wants it; the place is checked on the loaded stream."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests import helpers

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]
CAP = 1024
CHUNK_MAX = 2048  # tiles a scan workgroup owns at a time at most (csrc/train_rules.h: sparse_geom_rule)
FORMS = [("flat", 8), ("flat", 16), ("weights", 8), ("weights", 16)]


def _random_words(n_bytes, alphabet, seed, lo=2, hi=9):
    rng = np.random.default_rng(seed)
    n = 2 * n_bytes // (lo + hi - 1)
    lens = rng.integers(lo, hi, size=n)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=int(off[-1]))]
    return np.ascontiguousarray(flat), off


def _site_words(slot, word):
    """`word` (it holds the one pair x y of the stream) behind a filler, so that its x stands at `slot` of tile 0."""
    at = word.index(b"x")
    start = slot - at
    assert start >= 0
    filler = [b"zw"] if start % 2 else []  # (three slots: the odd starts)
    filler += [b"q"] * ((start - 3 * len(filler)) // 2)
    words = filler + [word] + [b"q"] * 4
    assert sum(len(w) + 1 for w in filler) == start and sum(len(w) + 1 for w in words) <= CAP
    return words


def _last_slot_words():
    filler = [b"zw"] + [b"q"] * 400  # 3 + 800 slots; the word p x y ends the stream: y is the last token, its separator the last live slot
    return filler + [b"pxy"]


SITES = {
    "slot0": (_site_words(0, b"xyr"), 0),
    "slot510": (_site_words(510, b"pxyr"), 510),
    "slot511": (_site_words(511, b"pxyr"), 511),
    "slot512": (_site_words(512, b"pxyr"), 512),
    "last": (_last_slot_words(), 804),
    "dead_start": (_site_words(0, b"xy"), 0),
    "dead_seam": (_site_words(511, b"xy"), 511),
}


def _expect(flat, off, freq, n_merges):
    base = helpers.base_tokens(SP)
    exp = {"flat": oracle.train_flat(flat, off, len(base) + n_merges, 1, SP, return_ids=True)[2],
           "weights": oracle.train_flat(flat, off, len(base) + n_merges, 1, SP, return_ids=True, freq=freq)[2]}
    for ids in exp.values():
        for a in ids.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return {"flat": flat, "off": off, "freq": freq, "base": base, "exp": exp, "n_merges": n_merges}


def _case(flat, off, n_merges, seed=5):
    freq = np.random.default_rng(seed).integers(1, 5, size=len(off) - 1).astype(np.uint64)  # (frequencies above 1: tile_wbase / wfreq)
    return _expect(flat, off, freq, n_merges)


@pytest.fixture(scope="module")
def ties():
    return _case(*_random_words(64 << 10, b"abcde", 3), 150)


@pytest.fixture(scope="module")
def one_tile():
    return _case(*_random_words(700, b"abcdef", 7), 40)


@pytest.fixture(scope="module")
def long_stream():
    return _case(*_random_words(9 << 19, b"etaoin", 11), 40)


@pytest.fixture(scope="module")
def sites():
    return {name: _case(*helpers.flatten(words), 6, seed=13) for name, (words, _slot) in SITES.items()}


def _check(case, layout, wpb, options=None, x_slot=None):
    from yet_another_bpe import _native

    n_merges = case["n_merges"]
    with _native.Context() as ctx:
        for k, v in {"verify": 1, "split": 1, "full_wpb": wpb, **(options or {})}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(case["base"])
        ctx.load_words(case["flat"], case["off"], case["freq"] if layout == "weights" else None)
        loaded = ctx.stats()
        if x_slot is not None:  # the site is where the case wants it
            dump = ctx.stream_dump()
            assert dump["n_tiles"] == 1
            row = dump["tiles"][0]
            assert row[x_slot] == ord("x") and row[x_slot + 1] == ord("y"), (x_slot, row[max(0, x_slot - 4):x_slot + 6])
        left, right, merged, count = ctx.train(n_merges, 1)
        st = ctx.stats()
    ids = case["exp"][layout]
    what = (layout, wpb, options)
    print(what, {k: st[k] for k in ("sparse_merges", "sparse_launches", "scan_skip_launches", "scan_skip_pieces_taken")}, loaded["n_tiles"])
    assert len(left) == len(ids["left"]), what
    assert np.array_equal(left, ids["left"]) and np.array_equal(right, ids["right"]) and np.array_equal(merged, ids["merged"]), what
    assert np.array_equal(np.asarray(count, dtype=np.uint64), ids["count"]), what
    assert st["sparse_merges"] == len(left) and st["scan_skip_launches"] > 0, what
    st["tiles_loaded"] = loaded["n_tiles"]
    return st


@pytest.mark.parametrize("layout,wpb", FORMS)
def test_ties_in_batches(ties, layout, wpb):
    st = _check(ties, layout, wpb)
    assert st["sparse_launches"] < st["sparse_merges"]  # batches above one merge


@pytest.mark.parametrize("layout,wpb", FORMS)
def test_ties_one_merge_per_launch(ties, layout, wpb):
    _check(ties, layout, wpb, {"batch_max": 1})


@pytest.mark.parametrize("layout,wpb", FORMS)
def test_stream_of_one_tile(one_tile, layout, wpb):
    assert _check(one_tile, layout, wpb)["tiles_loaded"] == 1


@pytest.mark.parametrize("steal", [0, 1])
@pytest.mark.parametrize("layout,wpb", FORMS)
def test_second_round_of_chunks(long_stream, layout, wpb, steal):
    st = _check(long_stream, layout, wpb, {"full_skip_blocks": 2, "chunk_steal": steal})
    assert st["tiles_loaded"] > 2 * CHUNK_MAX  # more than the two scan workgroups own in one round
    assert (st["scan_skip_pieces_taken"] > 0) == (steal == 1 and wpb == 8), (layout, wpb, steal, st["scan_skip_pieces_taken"])


@pytest.mark.parametrize("name", list(SITES))
@pytest.mark.parametrize("layout,wpb", FORMS)
def test_single_site_places(sites, name, layout, wpb):
    _check(sites[name], layout, wpb, x_slot=SITES[name][1])
