"""CPU (-m "not gpu"): the plain-Python trainer with a maximum token length (tests/limit_helpers.py) against the oracle where
no limit is set, the facts that pin it where one is, and the validation of BBPETrainerConfig.max_token_length."""
from __future__ import annotations

import pytest

from oracle import oracle
from tests import helpers, limit_helpers as lh


def test_no_limit_equals_the_oracle_on_the_golden_cases():
    for c in helpers.golden_cases():
        base = helpers.base_tokens(c["special_tokens"])
        vocab, merges = lh.train(c["words_b"], None, max(0, c["vocab_size"] - len(base)), c["min_frequency"], c["special_tokens"])
        exp_vocab, exp_merges = oracle.merge_loop(c["words_b"], c["vocab_size"], c["min_frequency"], c["special_tokens"])
        assert merges == exp_merges, c["name"]
        assert vocab == exp_vocab, c["name"]


def test_no_limit_equals_the_oracle_on_corpus_en():
    vocab, merges, trace = lh.en_model(None)
    exp_vocab, exp_merges = oracle.merge_loop(list(lh.en_words()), 257 + 400, 2, lh.SP)
    assert len(merges) == 400 and trace["stop"] == "cap"
    assert merges == exp_merges and vocab == exp_vocab


def test_the_input():
    uw, _fq = helpers.pooled(lh.en_words())
    assert len(lh.en_words()) == 6000
    assert len(uw) == 1624
    assert max(len(w) for w in uw) == 17


def test_limit_2_stops_on_the_best_eligible_pair():
    _vocab, merges, trace = lh.en_model(2)
    assert len(merges) == 293
    assert all(len(l) + len(r) == 2 for l, r in merges)
    # min_frequency = 2 fired on the best ELIGIBLE pair while pairs over the limit still have higher counts
    assert trace["stop"] == "min_frequency"
    assert trace["best_eligible"] < 2 <= trace["best_ineligible"]
    assert trace["best_ineligible"] > trace["best_eligible"]


@pytest.mark.parametrize("limit,index", [(2, 11), (3, 11), (4, 72), (6, 148), (8, 173)])
def test_where_a_limit_first_bites(limit, index):
    _v, free, _t = lh.en_model(None)
    _v, merges, _t = lh.en_model(limit)
    assert lh.first_difference(merges, free) == index
    assert max(len(l) + len(r) for l, r in merges) <= limit
    assert len(free[index][0]) + len(free[index][1]) > limit  # the unlimited run's merge there is the first one over the limit


def test_limit_16_changes_nothing():
    vocab, free, _t = lh.en_model(None)
    assert max(len(l) + len(r) for l, r in free) == 12
    v16, m16, _t = lh.en_model(16)
    assert m16 == free and v16 == vocab


@pytest.mark.parametrize("limit,n_merges", [(2, 366), (3, 926), (4, 1491)])
def test_limits_run_out_of_eligible_pairs(limit, n_merges):
    _vocab, merges, trace = lh.en_model(limit, num_merges=1 << 20, min_frequency=1)
    assert len(merges) == n_merges
    assert trace["stop"] == "no_pairs" and trace["best_eligible"] == 0


def test_resumed_start_is_the_one_shot_run():
    """start_merges: replaying a limited run's first merges and going on under the same limit gives the rest of that run."""
    uw, fq = helpers.pooled(lh.en_words())
    vocab, merges, _t = lh.en_model(4)
    v2, rest = lh.train(uw, fq, 250, 2, lh.SP, limit=4, start_merges=merges[:150])
    assert merges[:150] + rest == merges and v2 == vocab


# ---------------------------------------------------------------- config validation (no device, no file)
def _trainer(value):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    return BBPETrainer(BBPETrainerConfig(vocab_size=300, special_tokens=lh.SP, max_token_length=value))


def test_config_field_is_last_and_defaults_to_none():
    from yet_another_bpe.trainer import BBPETrainerConfig

    cfg = BBPETrainerConfig(1000, 3, 2, 1 << 20, 7, ["x"])
    assert cfg.max_token_length is None and cfg.special_tokens == ["x"]
    assert BBPETrainerConfig(1000, 3, 2, 1 << 20, 7, ["x"], 8).max_token_length == 8
    assert "bytes" in BBPETrainerConfig.__doc__.lower() and "save_lossless" in BBPETrainerConfig.__doc__


@pytest.mark.parametrize("value", [0, 1, -1, -16, True, False, 4.0, "8", (4,)])
def test_bad_limits_raise_before_any_file_or_device(value, tmp_path):
    from yet_another_bpe.trainer import BBPEModel

    missing = tmp_path / "never_read.txt"  # (would be FileNotFoundError if the files were looked at first)
    tr = _trainer(value)
    with pytest.raises(ValueError, match="max_token_length"):
        tr.train([missing])
    with pytest.raises(ValueError, match="max_token_length"):
        tr.train([missing], batch_bytes=1 << 20)
    model = BBPEModel(vocab={t: i for i, t in enumerate(helpers.base_tokens(lh.SP))}, merges=[], special_tokens=lh.SP)
    with pytest.raises(ValueError, match="max_token_length"):
        tr.train_from(model, [missing])
    with pytest.raises(ValueError, match="max_token_length"):
        tr._merge_loop([[97, 98], [97, 98]])


@pytest.mark.parametrize("value", [None, 2, 16, 1 << 20])
def test_good_limits_pass_validation(value, tmp_path):
    from yet_another_bpe.trainer import max_token_bytes

    tr = _trainer(value)
    assert max_token_bytes(tr.config) == (value or 0)
    with pytest.raises(FileNotFoundError):  # validation passed: the next thing looked at is the file
        tr.train([tmp_path / "missing.txt"], batch_bytes=1 << 20)


def test_sharded_text_driver_validates_too(tmp_path):
    from yet_another_bpe import distributed
    from yet_another_bpe.trainer import BBPETrainerConfig

    cfg = BBPETrainerConfig(vocab_size=300, special_tokens=lh.SP, max_token_length=1)
    with pytest.raises(ValueError, match="max_token_length"):
        distributed.train_text_sharded(None, [tmp_path / "missing.txt"], cfg, 0, 1)
