"""GPU (-m gpu): the batched selection (select_eval) on the small tie-heavy corpora of tests/tie_helpers.py, in every form
that reaches it, bit-exact against the C oracle: merges, vocabulary ids and the count of every merge.  No tolerances.

What reaches which branch is a condition on the INPUT, checked on the CPU (tie_helpers.replay, tools/batch_sim.cpp through
tests/test_batch_rule.py) and asserted here before the device is asked:
  undecided tie comparison (cmp_pre8 == 2)   stems    batch_sim variant 3 counts them; variants 4 / 5 mismatch (test_batch_rule)
  window narrowing (delta >>= 2)             levels   > 128 distinct pairs within 16 of the top, <= 128 at the top
  no-window fallback                         plateau  > 128 distinct pairs tie at the top (best count >= 16; count 1 at unit frequencies)
  id reuse inside a batch (hit)              reuse    merged bytes that are a token already, behind a merge they share no token with
  min_frequency / num_merges inside a batch  stems    every cut point 1..48, every count level of the first 100 merges"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle
from tests import helpers, tie_helpers

pytestmark = pytest.mark.gpu

N_MERGES = 400
BATCHED = {"split": 1, "batch_max": 16, "cand_min_count": 1}
OPTION_SETS = [
    {"split": 1, "batch_max": 16},
    {"split": 1, "batch_max": 16, "cand_min_count": 1},
    {"split": 1, "batch_max": 1},
    {"split": 1, "batch_max": 2},
    {"split": 1, "batch_max": 3},
    {"split": 1, "batch_max": 8},
    {"split": 1, "fused": 0},
    {"split": 1, "full_wpb": 16},
    {"split": 1, "cand_target": 64, "check_interval": 3},
    {"split": 1, "cand_rebuild_every": 1},
    {},
]
LAYOUTS = ["flat", "weighted", "device_dedup"]
REUSE = [c[0] for c in tie_helpers.reuse_cases()]


@lru_cache(maxsize=None)
def corpus(name: str):
    """-> (word types, frequencies, specials)"""
    if name == "stems":
        return (*tie_helpers.stems_types(), ())
    if name == "plateau":
        return (*tie_helpers.plateau_types(), ())
    if name == "plateau_once":  # every type once: the same pairs at counts 1 and 2
        types, _ = tie_helpers.plateau_types()
        return types, (1,) * len(types), ()
    if name == "levels":
        return (*tie_helpers.levels_types(), ())
    for cname, types, freqs, specials in tie_helpers.reuse_cases():
        if cname == name:
            return types, freqs, specials
    raise KeyError(name)


@lru_cache(maxsize=None)
def steps(name: str):
    types, freqs, specials = corpus(name)
    return tuple(tie_helpers.replay(types, freqs, specials, N_MERGES))


@lru_cache(maxsize=None)
def expected(name: str, mult: int = 1, n_merges: int = N_MERGES, min_frequency: int = 1):
    """The oracle's (vocab, merges, id triples + counts): computed once per corpus, read-only afterwards."""
    types, freqs, specials = corpus(name)
    flat, off = helpers.flatten(list(types))
    fq = np.array(freqs, dtype=np.uint64) * np.uint64(mult)
    vocab, merges, ids = oracle.train_flat(flat, off, len(helpers.base_tokens(specials)) + n_merges, min_frequency, list(specials), return_ids=True, freq=fq)
    for a in ids.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, merges, ids


@lru_cache(maxsize=None)
def inputs(name: str, layout: str, mult: int = 1):
    """-> (flat, off, freq or None, dedup) as the layout loads them"""
    types, freqs, _ = corpus(name)
    if layout == "weighted":
        uw, fq = tie_helpers.stems_pooled(mult) if name == "stems" else (list(types), np.array(freqs, dtype=np.uint64) * np.uint64(mult))
        flat, off = helpers.flatten(uw)
        return flat, off, fq, False
    assert mult == 1
    if name in ("stems", "plateau", "levels"):
        words = getattr(tie_helpers, name)()  # every occurrence, shuffled
    else:
        words = [w for w, f in zip(types, freqs) for _ in range(f)]
        words = [words[i] for i in np.random.default_rng(7).permutation(len(words))]
    flat, off = helpers.flatten(words)
    return flat, off, None, layout == "device_dedup"


def load(ctx, name: str, layout: str, mult: int = 1):
    flat, off, freq, dedup = inputs(name, layout, mult)
    ctx.set_vocab(helpers.base_tokens(corpus(name)[2]))
    ctx.load_words(flat, off, freq, dedup=dedup)


def context(options):
    from yet_another_bpe import _native

    ctx = _native.Context()
    ctx.set_option("verify", 1)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def decode(specials, left, right, merged):
    toks = helpers.base_tokens(specials)
    merges = []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        merges.append((toks[l], toks[r]))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
        else:
            assert toks[m] == toks[l] + toks[r], "merged id does not name left + right"
    return {t: i for i, t in enumerate(toks)}, merges


def assert_equals_oracle(got, name, mult=1, n_merges=N_MERGES, min_frequency=1, upto=None, what=None):
    """got: (left, right, merged, count) of the device; the oracle's first `upto` merges (all of them by default)."""
    assert_equals(got, expected(name, mult, n_merges, min_frequency), corpus(name)[2], upto, what)


def assert_equals(got, want, specials=(), upto=None, what=None):
    """The comparison of assert_equals_oracle with the oracle's result handed in: want = (vocab, merges, ids) of
    oracle.train_flat(..., return_ids=True) on the corpus the device was given (tests/test_gpu_big_counts.py brings its own)."""
    vocab, merges, ids = want
    n = len(merges) if upto is None else upto
    left, right, merged, count = got
    assert len(left) == n, (what, len(left), n)
    for field, arr in (("left", left), ("right", right), ("merged", merged), ("count", count)):
        if not np.array_equal(arr, ids[field][:n]):
            k = int(np.flatnonzero(np.asarray(arr) != ids[field][:n])[0])
            raise AssertionError(f"{what}: {field} differs first at merge {k}: device {arr[k]} oracle {ids[field][k]}")
    v, m = decode(specials, left, right, merged)
    assert m == merges[:n], what
    if upto is None:
        assert v == vocab, what


def train_once(name, layout, options, mult=1, n_merges=N_MERGES, min_frequency=1):
    with context(options) as ctx:
        load(ctx, name, layout, mult)
        got = ctx.train(n_merges, min_frequency)
        return got, ctx.stats()


def batched_path_ran(options) -> bool:
    return options.get("split") == 1 and options.get("batch_max", 16) > 1 and options.get("fused", 1) != 0


def assert_batched_path_ran(stats, what):
    # launches that skipped tiles by their signatures (the sparse form), and fewer launches than merges: batches formed
    assert stats["scan_skip_launches"] > 0, (what, stats["scan_skip_launches"])
    assert 0 < stats["sparse_launches"] < stats["sparse_merges"], (what, stats["sparse_launches"], stats["sparse_merges"])


# ---------------------------------------------------------------- the inputs reach the branches (CPU conditions, asserted here)
def test_inputs_reach_the_branches():
    """Conditions on the inputs, from the plain-Python replay -- no device involved.  A seed that misses one is changed, not the bound."""
    st = steps("plateau")
    assert sum(1 for s in st if s["at_top"] > tie_helpers.WIN and s["count"] >= 16) >= 50  # no-window fallback, list attached
    st = steps("plateau_once")
    assert sum(1 for s in st if s["at_top"] > tie_helpers.WIN and s["count"] == 1) >= 50   # ... and on the count-1 plateau
    st = steps("levels")
    assert sum(1 for s in st if s["near"] > tie_helpers.WIN and s["at_top"] <= tie_helpers.WIN) >= 20  # the window is narrowed
    hits = [s for name in REUSE for s in steps(name) if s["hit"]]
    assert len(hits) >= 5                                # merged bytes that were a token already
    assert sum(1 for s in hits if s["apart"]) >= 3       # ... behind a merge they share no token with: rule (1) lets them into its batch
    st = steps("stems")[:100]
    assert len({s["count"] for s in st}) >= 10           # count levels for min_frequency to cut at
    assert sum(1 for a, b in zip(st, st[1:]) if b["count"] < a["count"] and b["apart"]) >= 5  # a lower level behind an independent merge


# ---------------------------------------------------------------- forced forms
def _forced(name, layout, mults=(1,)):
    for mult in mults:
        for options in OPTION_SETS:
            what = (name, layout, mult, options)
            got, stats = train_once(name, layout, options, mult)
            assert_equals_oracle(got, name, mult, what=what)
            if batched_path_ran(options):
                assert_batched_path_ran(stats, what)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_stems_forced_forms(layout):
    """Tokens that share their first eight bytes: the tie rule's "cannot tell".  Weighted also at 1000 x the frequencies,
    where the window's reach is cmax >> win_shift and not the batch limit."""
    _forced("stems", layout, (1, 1000) if layout == "weighted" else (1,))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_plateau_forced_forms(layout):
    """More than 128 distinct pairs tie at the top: no window, a batch of one found the plain way."""
    _forced("plateau", layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_levels_forced_forms(layout):
    """More than 128 distinct pairs close under a small top level: the window is narrowed until it fits."""
    _forced("levels", layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", REUSE)
def test_reuse_forced_forms(name, layout):
    """Merged bytes that are a token already: the merge takes that id, and the batch ends in front of it."""
    _forced(name, layout)


# ---------------------------------------------------------------- stops inside a batch
def test_num_merges_ends_inside_a_batch():
    """train(n) for every n in 1..48 is the first n merges: wherever the batches' ends fall, the limit cuts them."""
    with context(BATCHED) as ctx:
        load(ctx, "stems", "weighted")
        assert_equals_oracle(ctx.train(N_MERGES, 1), "stems", what="full run")
        for n in range(1, 49):
            load(ctx, "stems", "weighted")
            assert_equals_oracle(ctx.train(n, 1), "stems", upto=n, what=f"num_merges {n}")


def test_min_frequency_fails_inside_a_batch():
    """min_frequency at every count level of the first 100 merges, and one above it: the merges with count >= min_frequency."""
    counts = expected("stems")[2]["count"]
    levels = sorted({int(c) for c in counts[:100]})
    with context(BATCHED) as ctx:
        for c in levels:
            for mf in (c, c + 1):
                n = int(np.count_nonzero(counts >= mf))  # (the best count never rises: a prefix)
                load(ctx, "stems", "weighted")
                assert_equals_oracle(ctx.train(N_MERGES, mf), "stems", upto=n, what=f"min_frequency {mf}")


def test_two_calls_split_anywhere_equal_one():
    """train(k) then train(64 - k) on one load, k in 1..32: the second call starts where a batch was cut."""
    with context(BATCHED) as ctx:
        for k in range(1, 33):
            load(ctx, "stems", "weighted")
            a = ctx.train(k, 1)
            b = ctx.train(64 - k, 1)
            assert ctx.verify_table() == 0, k
            assert_equals_oracle(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), "stems", upto=64, what=f"{k} + {64 - k}")


# ---------------------------------------------------------------- run to exhaustion
@pytest.mark.parametrize("options", [{}, BATCHED], ids=["default", "batched"])
@pytest.mark.parametrize("name", ["plateau", "plateau_once"] + REUSE)
def test_run_to_exhaustion(name, options):
    """min_frequency 1 until no pair is left: the low plateaus at the end of a job (count 1 at unit frequencies) are walked too."""
    n_all = 4096
    _vocab, merges, _ids = expected(name, 1, n_all, 1)
    assert 0 < len(merges) < n_all  # (the corpus ran out of pairs, not the limit)
    for layout in ("weighted", "flat"):
        got, _stats = train_once(name, layout, options, n_merges=n_all)
        assert_equals_oracle(got, name, 1, n_all, 1, what=(name, layout, options))
