"""GPU (-m gpu): every role of the sparse launch (k_scan_skip) finds its parameters.  One kernel serves the scan workgroups,
the lexrank riders, the long words' riders and, in its last workgroup, the flush's selection; the groups of parameters
that the candidate-tile loop does not touch are read from the kernel's argument segment by the role that needs them
(kernarg_read in csrc/yabpe_kernels.h), by their byte offsets.  A wrong offset shows as a wrong model: every case goes
through the public training call with the sparse form forced from the first merge (split = 1) and is compared bit for bit
with the C oracle -- ids and counts of every merge -- under verify = 1 (the incremental pair table equals a recount).

One corpus of ~5,000 tiles for all cases: random words of 2-12 letters with words that are exactly one pair, runs of one
letter and alternating letters mixed in (the general rewrite), and 36 words of 64-300 tokens (apply_long_block rides).
Flat and weighted (a frequency per word); 8- and 16-wave workgroups; a stream of more chunks than scan workgroups
(full_skip_blocks = 2) dealt by index and taken from the counter; the host looking at the state after every launch and
every 32, under a table that starts at 2^10 slots and grows."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle
from tests import helpers

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]
N_MERGES = 120
CHUNK_MAX = 2048  # tiles a workgroup sweeps at a time at most
N_LONG = 36


def _corpus():
    rng = np.random.default_rng(29)
    n_short = 600_000
    lens = rng.integers(2, 13, size=n_short)
    kind = rng.random(n_short)
    lens[kind < 0.04] = 2
    # the long words stand all through the stream
    at = np.sort(rng.choice(n_short, size=N_LONG, replace=False))
    lens[at] = rng.integers(64, 301, size=N_LONG)
    kind[at] = 1.0
    off = np.zeros(n_short + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    word_of = np.repeat(np.arange(n_short), lens)
    pos = np.arange(total) - np.repeat(off[:-1].astype(np.int64), lens)
    letters = np.frombuffer(b"etaoinshrdlu", dtype=np.uint8)
    p = np.array([12, 9, 8, 8, 7, 7, 6, 6, 6, 4, 4, 3], dtype=np.float64)
    flat = letters[rng.choice(len(letters), size=total, p=p / p.sum())]
    k = kind[word_of]
    flat[(k >= 0.04) & (k < 0.08)] = ord("e")                                            # aaaa...
    alt = (k >= 0.08) & (k < 0.12)                                                       # abab...
    flat[alt] = np.where(pos[alt] % 2 == 0, ord("t"), ord("a")).astype(np.uint8)
    two = k < 0.04                                                                       # the word IS the pair
    flat[two] = np.where(pos[two] == 0, ord("t"), ord("a")).astype(np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


@pytest.fixture(scope="module")
def case():
    flat, off = _corpus()
    freq = np.random.default_rng(5).integers(1, 4, size=len(off) - 1).astype(np.uint64)
    base = helpers.base_tokens(SP)
    exp = {"flat": oracle.train_flat(flat, off, len(base) + N_MERGES, 1, SP, return_ids=True)[2],
           "weights": oracle.train_flat(flat, off, len(base) + N_MERGES, 1, SP, return_ids=True, freq=freq)[2]}
    for ids in exp.values():
        for a in ids.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return {"flat": flat, "off": off, "freq": freq, "base": base, "exp": exp}


def _check(case, layout, options):
    from yet_another_bpe import _native

    with _native.Context() as ctx:
        for k, v in {"verify": 1, "split": 1, **options}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(case["base"])
        ctx.load_words(case["flat"], case["off"], case["freq"] if layout == "weights" else None)
        tiles_loaded = ctx.stats()["n_tiles"]
        left, right, merged, count = ctx.train(N_MERGES, 1)
        st = ctx.stats()
    ids = case["exp"][layout]
    what = (layout, options)
    print(what, {k: st[k] for k in ("sparse_merges", "scan_skip_launches", "scan_skip_pieces_taken", "n_long_words", "table_rebuilds")}, tiles_loaded)
    assert len(left) == N_MERGES == len(ids["left"]), what
    assert np.array_equal(left, ids["left"]) and np.array_equal(right, ids["right"]) and np.array_equal(merged, ids["merged"]), what
    assert np.array_equal(np.asarray(count, dtype=np.uint64), ids["count"]), what
    assert st["sparse_merges"] == N_MERGES and st["scan_skip_launches"] > 0, what
    assert st["n_long_words"] == N_LONG, what  # (the long words' riders ran in every case)
    st["tiles_loaded"] = tiles_loaded
    return st


@pytest.mark.parametrize("layout", ["flat", "weights"])
@pytest.mark.parametrize("wpb", [8, 16])
def test_scan_riders_and_tail_in_one_round(case, layout, wpb):
    st = _check(case, layout, {"full_wpb": wpb})
    assert st["tiles_loaded"] > 2 * CHUNK_MAX  # "a few thousand tiles"
    assert st["scan_skip_pieces_taken"] == 0
    assert st["sparse_launches"] < st["sparse_merges"]  # batches formed: the tail selected several merges at once


@pytest.mark.parametrize("steal", [0, 1])
def test_more_chunks_than_scan_workgroups(case, steal):
    st = _check(case, "flat", {"full_skip_blocks": 2, "full_wpb": 8, "chunk_steal": steal})
    assert st["tiles_loaded"] > 2 * CHUNK_MAX, "the stream must be longer than one round of chunks"
    assert (st["scan_skip_pieces_taken"] > 0) == (steal == 1)


@pytest.mark.parametrize("layout", ["flat", "weights"])
@pytest.mark.parametrize("interval", [1, 32])
def test_host_checks_and_table_growth(case, layout, interval):
    st = _check(case, layout, {"check_interval": interval, "table_min_log2": 10, "table_load_pct": 1})
    assert st["table_rebuilds"] > 0, (layout, interval)
