"""GPU (-m gpu): the branches of the training driver (yabpe_train's steps over one run state, csrc/train_rules.h) on small
inputs on which each of them fires.  The other suites pin the models; this file pins that a branch is taken -- the counter
that proves it is non-zero -- and gives the model of oracle.train_flat bit for bit: ids and counts of every merge, the
vocabulary, nothing left out.  Every context runs with verify = 1 (the incremental pair table equals a recount).

Two corpora, flat and weighted: `stems` of tests/tie_helpers.py (tie-heavy: batches form) with three words of 64 tokens and
more (the long-word path), and the pre-tokens of the first 200 KiB of tests/golden/corpus.en.

Not here: the sparse launch's second round in pieces (scan_skip_pieces_taken > 0).  It needs a stream of more tiles than one
round of chunks covers -- with full_skip_blocks = 2 more than 4,096 tiles, some four million tokens -- and
tests/test_gpu_steal.py asserts it at that size; full_skip_blocks = 2 runs here for the model alone."""
from __future__ import annotations

import random
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle, pretok
from tests import helpers, tie_helpers
from tests.test_gpu_batch_ties import assert_equals

pytestmark = pytest.mark.gpu

SP = ["<|endoftext|>"]
N_MERGES = {"stems": 160, "en": 300}


@lru_cache(maxsize=None)
def words(name: str) -> tuple[bytes, ...]:
    if name == "stems":
        rng = random.Random(77)
        long_words = [bytes(rng.choice(b"abcdef") for _ in range(n)) for n in (64, 130, 300)]
        return tuple(tie_helpers.stems() + long_words * 3)
    data = (helpers.GOLDEN / "corpus.en").read_bytes()[:200 << 10]
    return tuple(bytes(w) for w in pretok.pretokenize(data, SP))


@lru_cache(maxsize=None)
def inputs(name: str, layout: str):
    if layout == "weighted":
        uw, fq = helpers.pooled(words(name))
        return (*helpers.flatten(uw), fq)
    return (*helpers.flatten(list(words(name))), None)


@lru_cache(maxsize=None)
def expected(name: str):
    """The oracle's model, computed once per corpus (the layouts give the same one), read-only afterwards."""
    flat, off, fq = inputs(name, "weighted")
    vocab, merges, ids = oracle.train_flat(flat, off, len(helpers.base_tokens(SP)) + N_MERGES[name], 1, SP, return_ids=True, freq=fq)
    for a in ids.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, merges, ids


def train(name: str, layout: str, options: dict, calls=None, comm: bool = False):
    """-> ((left, right, merged, count), stats); calls: the merges of each yabpe_train call (default: one call)."""
    from yet_another_bpe import _native

    flat, off, fq = inputs(name, layout)
    with _native.Context(0) as ctx:
        ctx.set_option("verify", 1)
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_vocab(helpers.base_tokens(SP))
        if comm:
            ctx.comm_init(0, 1, _native.Context.comm_unique_id())
        ctx.load_words(flat, off, fq)
        parts = [ctx.train(n, 1) for n in (calls or [N_MERGES[name]])]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(4)), ctx.stats()


def check(name, layout, options, counters=(), **kw):
    got, st = train(name, layout, options, **kw)
    what = (name, layout, options)
    print(what, {k: st[k] for k in ("merges_done", "dense_merges", "sparse_merges", "scan_skip_launches", "fused_launches", "table_rebuilds",
                                    "retiles", "exchanges", "exchange_growths", "n_tiles", "n_long_words", "cand_rebuilds", "cand_rescans")})
    assert_equals(got, expected(name), SP, what=what)
    for c in counters:
        assert st[c] > 0, (what, c, st[c])
    return st


LAYOUTS = ["flat", "weighted"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name,split_pct", [("stems", 3000), ("en", 400)])
def test_form_switch_in_the_middle_of_a_call(name, layout, split_pct):
    check(name, layout, {"split": -1, "split_pct": split_pct}, ["dense_merges", "sparse_merges", "scan_skip_launches"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("options", [{"full_skip_blocks": 2}, {"chunk_steal": 0}, {"full_wpb": 16}, {"batch_max": 1}, {"batch_max": 16}], ids=str)
def test_sparse_launch_shapes(layout, options):
    st = check("stems", layout, {"split": 1, **options}, ["sparse_merges", "scan_skip_launches"])
    if options.get("batch_max") == 16:
        assert st["sparse_launches"] < st["sparse_merges"]  # batches formed


@pytest.mark.parametrize("name", ["stems", "en"])
def test_table_growth_and_rebuild(name):
    # (the load leaves a table of 2^10 slots and more at most half full, and these few merges add few pairs: the load
    # bound of 30 % is lowered to 1 % so that the first housekeeping already grows it; a rebuild after HALT_TABLE_FULL /
    # HALT_DELTA_FULL is test_one_rank_communicator's)
    check(name, "flat", {"table_min_log2": 10, "table_load_pct": 1}, ["table_rebuilds"])
    check(name, "weighted", {"table_min_log2": 10, "table_load_pct": 1, "split": 1}, ["table_rebuilds", "sparse_merges"])


@pytest.mark.parametrize("name", ["stems", "en"])
def test_retile(name):
    check(name, "flat", {"retile_min_tiles": 2}, ["retiles"])
    check(name, "flat", {"retile_min_tiles": 2, "split": 1}, ["retiles", "sparse_merges"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("options", [{"fused": 0}, {"cand_argmax": 0}, {"rank_rides": 0}, {"fused": 0, "split": 1}, {"rank_rides": 0, "split": 1}], ids=str)
def test_unfused_forms(layout, options):
    st = check("stems", layout, options)
    if options.get("fused") == 0 or options.get("cand_argmax") == 0:
        assert st["fused_launches"] == 0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_rank_communicator(layout):
    # delta_cap at its smallest: a merge leaves more records than an exchange transmits (HALT_DELTA_FULL), the size steps up
    check("stems", layout, {"force_comm": 1, "delta_cap": 1}, ["exchanges", "exchange_growths", "table_rebuilds"], comm=True)
    check("en", layout, {"force_comm": 1, "split": -1, "split_pct": 400}, ["exchanges", "sparse_merges"], comm=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_on_one_context_equal_one(layout):
    # (the second call enters with rec_base > 0 and no pending batch)
    check("stems", layout, {}, calls=[70, 90])
    check("stems", layout, {"split": 1}, ["sparse_merges"], calls=[70, 90])


@pytest.mark.parametrize("name", ["stems", "en"])
def test_u32_loop(name):
    check(name, "flat", {"id_bits": 32, "table_min_log2": 10, "retile_min_tiles": 2}, ["table_rebuilds", "retiles"])
    check(name, "weighted", {"id_bits": 32, "table_min_log2": 10, "retile_min_tiles": 2}, calls=[N_MERGES[name] // 2, N_MERGES[name] - N_MERGES[name] // 2])


def test_long_words_ride_and_run_on_their_own():
    for options in ({}, {"fused": 0}, {"split": 1}, {"split": 1, "fused": 0}):
        assert check("stems", "flat", options, ["n_long_words"])["n_long_words"] == 9
