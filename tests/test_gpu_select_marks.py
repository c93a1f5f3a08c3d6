"""GPU (-m gpu): the duplicate-free candidate list ("listed" bit per table slot, cand_note / k_cand_rebuild) and the window
cut from it by ballots (select_eval), bit-exact against the C oracle: merges, vocabulary ids and the count of every merge,
with the library's own table check on (verify = 1).  No tolerances.

The corpora, layouts and helpers are those of tests/test_gpu_batch_ties.py (tests/tie_helpers.py; the oracle's results are
computed once there and shared).  The option sets are the ones that move the list under the selection's feet: a rebuild at
every host check and none inside the run, a short list that is rebuilt often, a table that starts at 1,024 slots and grows
mid-run (the bitmap names slots: it has to follow), wide and narrow workgroups, batches of one and of sixteen, and the
selection as a launch of its own.

`flatline` is this file's own corpus: about a hundred word types of distinct bytes at frequencies within 4 % of each other,
so that between the ONE rebuild of its option set and the end of the run every pair a merge creates rises from nothing
past the list's threshold T -- the path through the bitmap's OR -- while the best count never comes near T (no second
rebuild).  That is a condition on the input, asserted on the CPU from a sequential replay before the device is asked; T is
taken from the options that fix it (cand_margin_max_pct 20 pins the margin, check_interval 4 the merge at which the list is
built), not from the code under test.

What no corpus can do: take a pair's count over T, under it and over it again between two rebuilds.  In sequential BPE a
token is created by exactly one merge (two pairs with the same bytes, (a, bc) after (ab, c), cannot both occur: whichever of
(a, b) and (b, c) is merged first is merged everywhere), so once both tokens of a pair exist its count only falls.  A
search over 4,500 random small corpora, with and without specials, found no pair whose count rose after it had fallen.  On
the device only the deltas of ONE launch, arriving in any order, can cross twice; that order cannot be forced.  The rule
itself -- a second crossing does not list again -- is pinned on the CPU model (tests/test_select_logic_model.py)."""
from __future__ import annotations

import random
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle
from tests import helpers, tie_helpers
from tests import test_gpu_batch_ties as ties

pytestmark = pytest.mark.gpu

N_MERGES = ties.N_MERGES  # 400
NO_REBUILD = 1 << 30
OPTION_SETS = [
    {"split": 1, "cand_rebuild_every": 1},
    {"split": 1, "cand_rebuild_every": NO_REBUILD},
    {"split": 1, "cand_target": 64, "check_interval": 3},
    {"split": 1, "table_min_log2": 10, "table_load_pct": 1},
    {"split": 1, "full_wpb": 8},
    {"split": 1, "full_wpb": 16},
    {"split": 1, "batch_max": 1},
    {"split": 1, "batch_max": 16, "cand_min_count": 1},
    {"split": 1, "fused": 0},
]
NAMES = ["stems", "levels", "plateau"] + ties.REUSE


@pytest.mark.parametrize("layout", ties.LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_list_moves_under_the_selection(name, layout):
    for options in OPTION_SETS:
        what = (name, layout, options)
        got, stats = ties.train_once(name, layout, options)
        ties.assert_equals_oracle(got, name, what=what)
        if ties.batched_path_ran(options):
            ties.assert_batched_path_ran(stats, what)
        if "table_load_pct" in options and name in ("stems", "levels", "plateau"):
            assert stats["table_rebuilds"] > 0, (what, stats["table_rebuilds"])  # the table did grow mid-run


# ---------------------------------------------------------------- flatline: crossings between two rebuilds
FLAT_MERGES = 200
FLAT_CHECK = 4
FLAT_MARGIN_PCT = 20
FLAT_OPTIONS = {"split": 1, "batch_max": 16, "cand_min_count": 1, "cand_rebuild_every": NO_REBUILD, "cand_margin_max_pct": FLAT_MARGIN_PCT,
                "check_interval": FLAT_CHECK}


@lru_cache(maxsize=None)
def flatline_types(seed: int = 71):
    rng = random.Random(seed)
    types: list[bytes] = []
    used: set[bytes] = set()
    while len(types) < 100:
        w = bytes(rng.sample(range(33, 250), rng.randint(4, 7)))  # (distinct bytes inside a word: no a == b runs)
        pairs = {w[j:j + 2] for j in range(len(w) - 1)}
        if not pairs & used:  # (no byte pair in two types: every pair's count is one type's frequency)
            used |= pairs
            types.append(w)
    return tuple(types), tuple(1000 + rng.randrange(0, 41) for _ in types)


@lru_cache(maxsize=None)
def flatline_counts():
    """Sequential BPE, a full recount per step -> [(best count, {pair: count})] before each of the first FLAT_MERGES merges."""
    types, freqs = flatline_types()
    words = [[bytes([b]) for b in w] for w in types]
    out = []
    for _ in range(FLAT_MERGES):
        pc: Counter = Counter()
        for w, f in zip(words, freqs):
            for j in range(len(w) - 1):
                pc[(w[j], w[j + 1])] += f
        (x, y), cnt = max(pc.items(), key=lambda kv: (kv[1], kv[0]))
        out.append((cnt, dict(pc)))
        for w in words:
            j = 0
            while j + 1 < len(w):
                if w[j] == x and w[j + 1] == y:
                    w[j:j + 2] = [x + y]
                j += 1
    return out


def threshold(best: int) -> int:
    """T of a list built at best count `best` with the margin pinned at FLAT_MARGIN_PCT (cand_rebuild, yabpe.hip)."""
    margin = max(1, int(best * (FLAT_MARGIN_PCT / 100.0)))
    return best - min(margin, best - 1)


@lru_cache(maxsize=None)
def flatline_expected():
    types, freqs = flatline_types()
    flat, off = helpers.flatten(list(types))
    vocab, merges, ids = oracle.train_flat(flat, off, len(helpers.base_tokens(())) + FLAT_MERGES, 1, [], return_ids=True, freq=np.array(freqs, dtype=np.uint64))
    for a in ids.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return vocab, merges, ids


def test_flatline_crosses_between_rebuilds_on_the_cpu():
    """The condition on the input -- no device involved.  A seed that misses it is changed, not the bound."""
    st = flatline_counts()
    assert len(st) == FLAT_MERGES
    best0, best_end = st[0][0], st[-1][0]
    # the list is built at the first host check behind a merge: merge FLAT_CHECK, from the count of the merge selected last
    # (FLAT_CHECK - 1 or FLAT_CHECK: whether one is pending) -- both thresholds are carried through
    ts = {threshold(st[FLAT_CHECK - 1][0]), threshold(st[FLAT_CHECK][0])}
    for T in ts:
        listed = sum(1 for c in st[FLAT_CHECK][1].values() if c >= T)
        # the margin stays pinned: not halved (more than cand_target = 768 pairs listed); doubling is capped by the option
        assert listed <= 768
        # no second rebuild, whatever the cadence of the host's checks: the best count stays clear of T + 2 x (its largest
        # possible drop between two checks) + 1 (cand_rebuild_rule), and the list stays under 960 entries
        assert best_end >= T + 2 * (best0 - best_end) + 2
        crossings = 0
        for k in range(FLAT_CHECK + 1, FLAT_MERGES):
            before, now = st[k - 1][1], st[k][1]
            crossings += sum(1 for p, c in now.items() if c >= T and before.get(p, 0) < T)
        assert crossings >= 100, crossings            # pairs that rise from under T past it while that one list lives
        assert listed + crossings <= 960, (listed, crossings)
    # a pair's count never rises after it has fallen (module docstring): between two rebuilds no pair crosses T twice
    for T in ts:
        up = Counter()
        for k in range(1, FLAT_MERGES):
            before, now = st[k - 1][1], st[k][1]
            for p, c in now.items():
                if c >= T and before.get(p, 0) < T:
                    up[p] += 1
        assert max(up.values()) == 1


@pytest.mark.parametrize("layout", ties.LAYOUTS)
def test_flatline_crossings_between_rebuilds(layout):
    test_flatline_crosses_between_rebuilds_on_the_cpu()  # (asserted before the device is asked, also when run alone)
    types, freqs = flatline_types()
    if layout == "weighted":
        flat, off = helpers.flatten(list(types))
        freq, dedup = np.array(freqs, dtype=np.uint64), False
    else:
        words = [w for w, f in zip(types, freqs) for _ in range(f)]
        words = [words[i] for i in np.random.default_rng(7).permutation(len(words))]
        flat, off = helpers.flatten(words)
        freq, dedup = None, layout == "device_dedup"
    for options in (FLAT_OPTIONS, {**FLAT_OPTIONS, "cand_rebuild_every": 1}):
        with ties.context(options) as ctx:
            ctx.set_vocab(helpers.base_tokens(()))
            ctx.load_words(flat, off, freq, dedup=dedup)
            got = ctx.train(FLAT_MERGES, 1)
            stats = ctx.stats()
        ties.assert_equals(got, flatline_expected(), (), what=("flatline", layout, options))
        ties.assert_batched_path_ran(stats, ("flatline", layout, options))
        if options["cand_rebuild_every"] == NO_REBUILD:
            assert stats["cand_rebuilds"] == 1, stats["cand_rebuilds"]  # ONE list for the whole run, as the CPU condition says
