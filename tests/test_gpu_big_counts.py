"""GPU (-m gpu): training at word frequencies up to 2^32-1 and pair counts past 2^32 (corpora of tests/big_count_helpers.py),
bit-exact against the C oracle: left / right / merged ids, the 64-bit count of every merge, merges and vocabulary.  No
tolerances.  The oracle itself is pinned to a recount on Python integers in tests/test_big_counts_model.py, which also
asserts what these inputs reach: in each `small` seed more than 90 of the first 150 steps have a best count >= 2^32 whose
low 32 bits point at ANOTHER pair, so a narrowing to 32 bits anywhere between a word's frequency and the returned count
(an LDS add, a wave reduction, the flush, the long-word rewrite, the resumed load, the exchange, the selection window,
whose reach is capped at 2^31 only when the best count is above 2^32) selects another merge or returns another count.

Every context runs with verify = 1; the forms are forced by options as in tests/test_gpu_batch_ties.py, whose comparison
(assert_equals) is used here.  The two-rank case is the `huge_weights` scenario of tests/test_gpu_distributed.py."""
from __future__ import annotations

import numpy as np
import pytest

from tests import big_count_helpers as bc
from tests import helpers
from tests.test_gpu_batch_ties import assert_batched_path_ran, assert_equals, batched_path_ran, context

pytestmark = pytest.mark.gpu

SMALL = [f"small{s}" for s in bc.SMALL_SEEDS]
BATCHED = {"split": 1, "batch_max": 16, "cand_min_count": 1}
SMALL_OPTIONS = [
    {},
    {"split": 0},
    {"split": 1},
    BATCHED,
    {**BATCHED, "fused": 0},
    {"split": 1, "batch_max": 1},
    {"split": 1, "batch_max": 3},
    {"split": 1, "full_wpb": 16},
    {"split": 1, "cand_target": 64, "check_interval": 3},
    {"split": 1, "cand_rebuild_every": 1},
    {"cand_argmax": 0},
]
TILES_OPTIONS = [
    {},
    {"split": 1},
    {"split": 1, "full_wpb": 16},
    {"split": 1, "batch_max": 8, "check_interval": 3},
    {"split": 0},
    {"table_min_log2": 10, "check_interval": 7},  # the table passes 30 % load on the way: growth and k_rehash carry the large counts
]
LONG_OPTIONS = [{}, {"split": 1}, {"long_sig": 0}]
BASE = helpers.base_tokens(())


def ident(options) -> str:
    return ",".join(f"{k}={v}" for k, v in options.items()) or "default"


def load(ctx, types, freqs):
    flat, off = helpers.flatten(list(types))
    ctx.set_vocab(BASE)
    ctx.load_words(flat, off, bc.freq_array(freqs))


def train_named(ctx, name, n_merges, min_frequency=1):
    """Loads the named corpus (weighted), trains, compares with the oracle and requires a clean table."""
    load(ctx, *bc.named(name))
    got = ctx.train(n_merges, min_frequency)
    assert_equals(got, bc.expected(name, n_merges, min_frequency), what=(name, n_merges, min_frequency))
    assert ctx.verify_table() == 0, name
    return got


# ---------------------------------------------------------------- forced forms, one tile
@pytest.mark.parametrize("options", SMALL_OPTIONS, ids=ident)
def test_small_forced_forms(options):
    with context(options) as ctx:
        for name in SMALL:
            got = train_named(ctx, name, 400)
            assert len(got[0]) == 400 and int(got[3][0]) > 1 << 36
            if batched_path_ran(options):
                assert_batched_path_ran(ctx.stats(), (name, options))


# ---------------------------------------------------------------- many tiles
@pytest.mark.parametrize("options", TILES_OPTIONS, ids=ident)
def test_many_tiles(options):
    """20,000 types, 187 tiles: every one of the 600 counts is at least 2^32 and sums over many tiles and workgroups."""
    with context(options) as ctx:
        got = train_named(ctx, "tiles", 600)
        stats = ctx.stats()
    assert len(got[0]) == 600 and int(got[3].min()) >= 1 << 32
    assert stats["n_tiles"] > 100
    if options.get("split") == 1:
        assert stats["scan_skip_launches"] > 0, stats["scan_skip_launches"]
    if "table_min_log2" in options:
        # the load leaves 2^16 slots and zero rebuilds behind: the table grew during the merges (k_rehash moved counts >= 2^32)
        assert stats["table_rebuilds"] >= 1 and stats["table_capacity"] > 1 << 16, (stats["table_rebuilds"], stats["table_capacity"])


# ---------------------------------------------------------------- long words
@pytest.mark.parametrize("options", LONG_OPTIONS, ids=ident)
def test_long_words(options):
    """Runs of one letter (a == b), words past one 1,024-token chunk of the long-word rewrite, both sides of the 63 / 64
    limit, at frequencies up to 2^32-1."""
    types, _freqs = bc.named("long")
    with context(options) as ctx:
        train_named(ctx, "long", 200)
        assert ctx.stats()["n_long_words"] == sum(1 for w in types if len(w) >= 64) == 9


# ---------------------------------------------------------------- the stop rule at a large count
@pytest.mark.parametrize("options", [{}, BATCHED], ids=["default", "batched"])
def test_min_frequency_above_2_33(options):
    with context(options) as ctx:
        for name in SMALL:
            mf = int(bc.expected(name, 400)[2]["count"][40]) + 1
            assert mf > 1 << 33
            got = train_named(ctx, name, 400, mf)
            assert len(got[0]) == 40


# ---------------------------------------------------------------- resume
def test_resumed_load_keeps_the_frequencies():
    from yet_another_bpe import _native

    types, freqs = bc.named("small1")
    flat, off = helpers.flatten(list(types))
    with context({}) as ctx:
        load(ctx, types, freqs)
        first = ctx.train(120, 1)
    assert len(first[0]) == 120
    toks, triples = _native.merge_triples(BASE, _native.decode_merges(BASE, *first[:3])[1])
    assert all(np.array_equal(a, b) for a, b in zip(triples, first[:3]))
    with context({}) as ctx:
        ctx.set_vocab(toks)
        ctx.load_words_resumed(flat, off, bc.freq_array(freqs), triples)
        assert ctx.verify_table() == 0
        second = ctx.train(280, 1)
        assert ctx.verify_table() == 0
    assert_equals(tuple(np.concatenate([a, b]) for a, b in zip(first, second)), bc.expected("small1", 400), what="120 + 280")


# ---------------------------------------------------------------- the limit of a frequency
def test_frequency_limit():
    from yet_another_bpe import _native

    types, freqs = bc.named("small1")
    assert freqs[0] == bc.F_MAX
    flat, off = helpers.flatten(list(types))
    over = bc.freq_array(freqs)
    over[0] = 1 << 32
    with context({}) as ctx:
        train_named(ctx, "small1", 400)  # 2^32-1 loads and trains
        ctx.set_vocab(BASE)
        with pytest.raises(_native.YabpeError) as e:
            ctx.load_words(flat, off, over)
        assert e.value.code == _native.E_CAPACITY and "exceeds 2^32-1" in str(e.value)
        train_named(ctx, "small1", 400)  # the context is still usable


# ---------------------------------------------------------------- through the pool
def test_through_the_pool():
    from yet_another_bpe import _native

    types, freqs = bc.named("small2")
    flat, off = helpers.flatten(list(types))
    fq = bc.freq_array(freqs)
    with context({}) as ctx:
        ctx.pool_add(flat, off, fq // np.uint64(2))
        ctx.pool_add(flat, off, fq - fq // np.uint64(2))
        items = ctx.pool_items()
        assert items == dict(zip(types, freqs))
        pb, po, pf, nu, _nb = ctx.pool_get()
        assert nu == len(types)
        ctx.set_vocab(BASE)
        ctx.load_words_ptr(pb, po, nu, freq_ptr=pf)
        got = ctx.train(400, 1)
        assert ctx.verify_table() == 0
        assert_equals(got, bc.oracle_run(list(items), list(items.values()), 400), what="pooled order")
        assert_equals(got, bc.expected("small2", 400), what="the order does not matter")
        # one more occurrence of a word that stands at 2^32-1: the pool counts on (64-bit), the load refuses
        w = types[0]
        assert items[w] == bc.F_MAX
        ctx.pool_add(*helpers.flatten([w]), np.array([1], dtype=np.uint64))
        before = ctx.pool_items()
        assert before == {**items, w: 1 << 32}
        pb, po, pf, nu, _nb = ctx.pool_get()
        with pytest.raises(_native.YabpeError) as e:
            ctx.load_words_ptr(pb, po, nu, freq_ptr=pf)
        assert e.value.code == _native.E_CAPACITY and "exceeds 2^32-1" in str(e.value)
        assert ctx.pool_items() == before
