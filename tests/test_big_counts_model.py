"""CPU: the references of tests/test_gpu_big_counts.py at word frequencies up to 2^32-1 and pair counts past 2^32
(corpora of tests/big_count_helpers.py).  The C oracle against a full recount on Python integers -- merges, vocabulary ids
and the count of every merge -- and the sequential model of the device layout (tests/hostmodel/tile_model.cpp) against the
oracle.  Then the conditions the device tests rely on: what the inputs reach, from the Python reference over the first 150
merges of each `small` seed.  A seed that misses a condition is a broken generator: the thresholds stay.

  condition                                                                   required   seeds 1, 2, 3
  merges with count >= 2^32                                                   >= 50      91, 98, 95
  steps where the maximum by (count mod 2^32, bytes) is not the true maximum  >= 50      91, 98, 95
      (a 32-bit truncation anywhere in counting or selection picks another merge there)
  steps with a second pair of count >= 2^32 within 2^31 of the best           >= 40      78, 83, 84
      (select_eval's window holds more than one entry while its cap of 2^31 binds)
  consecutive merges with equal counts >= 2^32                                >= 1       4, 1, 2
      (the tie-break by bytes at a large count)
  merges with count > count[40]                                               == 40      40, 40, 40
      (count[40] = 10737418235, 10737866652, 10737418239: above 2^33; min_frequency = count[40] + 1 stops after 40 merges)
  `tiles`: all 600 counts >= 2^32, the first 2^42.0; `long`: 9 types of 64 bytes or more, the first count 2^42.5"""
from __future__ import annotations

import pytest

from tests import big_count_helpers as bc
from tests.test_hostmodel import model_lib, run_model  # noqa: F401  (model_lib: the fixture that builds the model)

SMALL = [f"small{s}" for s in bc.SMALL_SEEDS]


def assert_oracle_equals_python(name, n_merges, min_frequency=1):
    types, freqs = bc.named(name)
    vocab, merges, ids = bc.expected(name, n_merges, min_frequency)
    py_vocab, py_merges, py_counts = bc.py_reference(types, freqs, n_merges, min_frequency)
    n = len(py_merges)
    assert merges == py_merges
    assert [int(c) for c in ids["count"]] == py_counts  # (Python integers on both sides: no rounding, no wrap)
    assert vocab == py_vocab
    toks = sorted(py_vocab, key=py_vocab.get)
    assert [toks[i] for i in ids["left"]] == [a for a, _ in py_merges] and [toks[i] for i in ids["right"]] == [b for _, b in py_merges]
    assert [toks[i] for i in ids["merged"]] == [a + b for a, b in py_merges]
    return n, py_counts


# ---------------------------------------------------------------- the generator is the one the thresholds were set for
def test_corpora_are_what_they_say():
    for name in SMALL:
        types, freqs = bc.named(name)
        assert len(types) == len(set(types)) == len(freqs) == 240
        assert all(2 <= len(w) <= 12 and set(w) <= set(b"abcde") for w in types)
        assert all(1 <= f <= bc.F_MAX for f in freqs)
        assert all(f == bc.F_MAX for f in freqs[0::6]) and all(bc.F_MAX - 1000 < f < bc.F_MAX for f in freqs[1::6])
        assert all(abs(f - (1 << 31)) <= 3 for f in freqs[2::6]) and all(f & (f - 1) == 0 for f in freqs[3::6])
    types, freqs = bc.named("tiles")
    assert len(set(types)) == 20000 and sum(len(w) for w in types) < 170_000  # (many tiles, a small input)
    types, freqs = bc.named("long")
    assert list(types[:9]) == bc.LONG_WORDS and list(freqs[:9]) == bc.LONG_FREQS and len(types) == len(set(types))
    assert sorted(len(w) for w in types if len(w) >= 63)[:3] == [64, 65, 185]  # both sides of the 63 / 64 limit ...
    assert max(len(w) for w in types if len(w) < 64) == 12                      # ... (the short side: the random words)
    assert sum(1 for w in types if len(w) > 1024) == 2                          # past one 1,024-token chunk


# ---------------------------------------------------------------- the oracle against Python integers
@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_python_integers_small(name):
    n, counts = assert_oracle_equals_python(name, 400)
    assert n == 400 and counts[0] > 1 << 36


def test_oracle_equals_python_integers_long():
    n, counts = assert_oracle_equals_python("long", 200)
    assert n == 200 and counts[0] > 1 << 42


def test_oracle_equals_python_integers_tiles():
    """The first 40 merges only (the Python loop recounts 20,000 types per merge); all 600 of the oracle's stay above 2^32."""
    n, counts = assert_oracle_equals_python("tiles", 40)
    assert n == 40 and counts[0] > 1 << 41
    _vocab, merges, ids = bc.expected("tiles", 600)
    assert len(merges) == 600 and int(ids["count"].min()) >= 1 << 32
    assert merges[:40] == bc.expected("tiles", 40)[1]


# ---------------------------------------------------------------- the model of the device layout against the oracle
@pytest.mark.parametrize("cap,lmax", [(1024, 64), (64, 16)])
@pytest.mark.parametrize("name", SMALL)
def test_tile_model_equals_oracle(model_lib, name, cap, lmax):  # noqa: F811
    types, freqs = bc.named(name)
    vocab, merges, _ids = bc.expected(name, 300)
    v, m = run_model(model_lib, list(types), bc.freq_array(freqs), 256 + 300, 1, (), cap, lmax, verify=1)
    assert m == merges and v == vocab


# ---------------------------------------------------------------- the inputs reach what they are meant to reach
@pytest.mark.parametrize("name", SMALL)
def test_inputs_reach_large_counts(name):
    c = bc.conditions(name)
    assert len(c["counts"]) == 150
    assert c["big"] >= 50
    assert c["low32_lies"] >= 50
    assert c["window"] >= 40
    assert c["big_ties"] >= 1


@pytest.mark.parametrize("name", SMALL)
def test_stop_rule(name):
    """min_frequency = count[40] + 1: the oracle stops after exactly the merges whose count is above count[40]."""
    counts = bc.conditions(name)["counts"]
    mf = counts[40] + 1
    assert mf > 1 << 33
    assert sum(1 for c in counts if c >= mf) == 40
    n, _ = assert_oracle_equals_python(name, 400, mf)
    assert n == 40
