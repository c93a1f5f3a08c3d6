"""GPU (-m gpu): BBPETrainer._run across the hand-over from the u16 to the u32 merge loop with the bound
lowered: trainer.U16_TOKENS is patched (monkeypatch) to the base tokens + h, so the u16 path is only asked for fewer merges
and the second context replays tens of merges instead of 65,278.  The default environment applies (YABPE_ID_BITS unset:
auto) unless a test says otherwise.  Expected models come from the C oracle, tests/limit_helpers.py and tie_helpers.replay;
the expected last_stats (id16_merges, id16_stages, id32_merges, id32_replayed_merges) from the reference's merge list by the
rule of stage1_merges (handover_helpers.expected_stages), never from the run.  Exact: merges, vocabulary and ids.
tests/test_id32_handover_inputs.py pins, on the CPU, what the inputs are chosen for."""
from __future__ import annotations

import numpy as np
import pytest

from tests import handover_helpers as hh
from tests import helpers, limit_helpers as lh
from yet_another_bpe import trainer
from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

pytestmark = pytest.mark.gpu
SP = hh.SP


@pytest.fixture
def bound(monkeypatch):
    """lower(n): trainer.U16_TOKENS = n for this test"""
    monkeypatch.delenv("YABPE_ID_BITS", raising=False)
    monkeypatch.delenv("YABPE_BATCH_BYTES", raising=False)
    monkeypatch.delenv("YABPE_LAYOUT", raising=False)

    def lower(n_tokens: int) -> int:
        monkeypatch.setattr(trainer, "U16_TOKENS", int(n_tokens))
        return int(n_tokens)

    return lower


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    return hh.write_file(tmp_path_factory.mktemp("handover") / "corpus.txt")


def count_contexts(monkeypatch, t: BBPETrainer) -> list:
    made, make = [], t._context

    def counted():
        made.append(1)
        return make()

    monkeypatch.setattr(t, "_context", counted)
    return made


def check_stats(t: BBPETrainer, base, merges, budget: int, u16: int, n_old: int = 0, mode: str = "auto") -> dict:
    want = hh.expected_stages(len(base), hh.fresh_flags(base, merges), budget, u16, n_old, mode)
    assert hh.picked(t.last_stats) == want, (hh.picked(t.last_stats), want)
    return want


# ---------------------------------------------------------------- 1. words level, tie-heavy
@pytest.mark.parametrize("h", [1, 17, 200])
@pytest.mark.parametrize("name", ["stems", "plateau", "levels"])
def test_tie_heavy_words(bound, name, h):
    types, freqs, (exp_vocab, exp_merges) = hh.tie_reference(name)
    u16 = bound(256 + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=256 + hh.TIE_BUDGET, min_frequency=1, special_tokens=[]))
    vocab, merges = t._merge_loop_words(types, np.array(freqs, dtype=np.uint64))
    assert merges == exp_merges and vocab == exp_vocab
    want = check_stats(t, helpers.base_tokens([]), exp_merges, hh.TIE_BUDGET, u16)
    assert want["id16_merges"] == h and want["id32_merges"] == len(exp_merges) - h


# ---------------------------------------------------------------- 2. stage 1 repeats after reused ids
@pytest.mark.parametrize("h", [10, 2])
@pytest.mark.parametrize("name", ["abc_many", "abcdef_pairs"])
def test_stage_one_repeats_after_reused_ids(bound, name, h):
    c = hh.reuse_case(name)
    u16 = bound(len(c["base"]) + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=c["vocab_size"], min_frequency=1, special_tokens=c["specials"]))
    vocab, merges = t._merge_loop_words(c["types"], np.array(c["freqs"], dtype=np.uint64))
    assert merges == c["merges"] and vocab == c["vocab"]
    # the three numbers from tie_helpers.replay: a hit takes no id, so stage 1 is asked again for the ids it left
    fresh = [k not in c["hits"] for k in range(c["n_steps"])]
    want = hh.expected_stages(len(c["base"]), fresh, c["budget"], u16)
    assert hh.picked(t.last_stats) == want
    absorbed = sum(1 for k in c["hits"] if k < want["id16_merges"])
    assert want["id16_merges"] == h + absorbed
    assert want["id16_stages"] >= 2 or (name, h) == ("abc_many", 2)  # (there the first hits are the second and third merge of stage 2)


# ---------------------------------------------------------------- 3. stop rules
def test_a_stop_inside_stage_one(bound, monkeypatch):
    types, freqs, (_v, ref) = hh.tie_reference("stems")
    min_frequency, j, h = hh.stop_points()["early"]
    u16 = bound(256 + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=256 + hh.TIE_BUDGET, min_frequency=min_frequency, special_tokens=[]))
    made = count_contexts(monkeypatch, t)
    vocab, merges = t._merge_loop_words(types, np.array(freqs, dtype=np.uint64))
    assert merges == ref[:j] and j < h and vocab == {tok: i for i, tok in enumerate(helpers.base_tokens([]) + [l + r for l, r in ref[:j]])}
    assert hh.picked(t.last_stats) == {"id16_merges": j, "id16_stages": 1, "id32_merges": 0, "id32_replayed_merges": 0}
    check_stats(t, helpers.base_tokens([]), ref[:j], hh.TIE_BUDGET, u16)
    assert len(made) == 1  # no u32 context


def test_a_stop_after_one_merge_of_stage_two(bound, monkeypatch):
    types, freqs, (_v, ref) = hh.tie_reference("stems")
    min_frequency, j, h = hh.stop_points()["seam"]
    u16 = bound(256 + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=256 + hh.TIE_BUDGET, min_frequency=min_frequency, special_tokens=[]))
    made = count_contexts(monkeypatch, t)
    vocab, merges = t._merge_loop_words(types, np.array(freqs, dtype=np.uint64))
    assert merges == ref[:j] and j == h + 1 and vocab == {tok: i for i, tok in enumerate(helpers.base_tokens([]) + [l + r for l, r in ref[:j]])}
    assert hh.picked(t.last_stats) == {"id16_merges": h, "id16_stages": 1, "id32_merges": 1, "id32_replayed_merges": h}
    check_stats(t, helpers.base_tokens([]), ref[:j], hh.TIE_BUDGET, u16)
    assert len(made) == 2


@pytest.mark.parametrize("past", [0, 1])
def test_a_budget_that_ends_at_the_bound(bound, monkeypatch, past):
    """len(toks) + num_merges == U16_TOKENS runs on the u16 path alone; one merge more is one merge of the u32 path."""
    types, freqs, (_v, ref) = hh.tie_reference("plateau")
    h = 30
    u16 = bound(256 + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=256 + h + past, min_frequency=1, special_tokens=[]))
    made = count_contexts(monkeypatch, t)
    vocab, merges = t._merge_loop_words(types, np.array(freqs, dtype=np.uint64))
    assert merges == ref[:h + past] and vocab == {tok: i for i, tok in enumerate(helpers.base_tokens([]) + [l + r for l, r in ref[:h + past]])}
    want = hh.expected_stages(256, hh.fresh_flags(helpers.base_tokens([]), ref[:h + past]), h + past, u16)
    if past:
        assert hh.picked(t.last_stats) == want == {"id16_merges": h, "id16_stages": 1, "id32_merges": 1, "id32_replayed_merges": h}
        assert len(made) == 2
    else:
        assert want is None and "id16_merges" not in t.last_stats and "id32_merges" not in t.last_stats
        assert t.last_stats["merges_done"] == h and len(made) == 1


# ---------------------------------------------------------------- 4. a maximum token length
def test_max_token_length(bound):
    uw, fq = helpers.pooled(lh.en_words())
    exp_vocab, exp_merges = hh.limit4_reference()
    base = helpers.base_tokens(lh.SP)
    u16 = bound(len(base) + 50)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=len(base) + 300, min_frequency=1, special_tokens=lh.SP, max_token_length=4))
    vocab, merges = t._merge_loop_words(uw, fq)
    assert merges == exp_merges and vocab == exp_vocab
    assert max(len(l + r) for l, r in merges) == 4
    check_stats(t, base, exp_merges, 300, u16)


# ---------------------------------------------------------------- 5. files through the device pre-tokeniser
def train_file(corpus_file, case: str, batch_bytes=None, n_merges: int = hh.FILE_MERGES):
    t = BBPETrainer(BBPETrainerConfig(vocab_size=257 + n_merges, **hh.FILE_CFG, **hh.FILE_CASES[case]))
    return t, t.train([corpus_file], batch_bytes=batch_bytes)


@pytest.mark.parametrize("case", list(hh.FILE_CASES))
def test_files_through_the_device_pretokeniser(bound, monkeypatch, corpus_file, case):
    """The second context loads device-pointer words that the first context owns."""
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    exp_vocab, exp_merges = hh.file_reference(corpus_file, **hh.FILE_CASES[case])
    base = helpers.base_tokens(SP)
    u16 = bound(len(base) + hh.FILE_H)
    t, model = train_file(corpus_file, case)
    assert model.merges == exp_merges and model.vocab == exp_vocab
    want = check_stats(t, base, exp_merges, hh.FILE_MERGES, u16)
    assert want["id16_merges"] >= hh.FILE_H and want["id32_merges"] == hh.FILE_MERGES - want["id16_merges"]


# ---------------------------------------------------------------- 6. batch_bytes
@pytest.mark.parametrize("case", ["gpt2_g3", "cl100k_nfc"])
def test_batched_file_gives_the_same_model(bound, monkeypatch, corpus_file, case):
    """The word pool is read by both stages' loads and cleared once, after the second."""
    from yet_another_bpe import _native

    exp_vocab, exp_merges = hh.file_reference(corpus_file, **hh.FILE_CASES[case])
    base = helpers.base_tokens(SP)
    u16 = bound(len(base) + hh.FILE_H)
    cleared = []
    clear = _native.Context.pool_clear
    monkeypatch.setattr(_native.Context, "pool_clear", lambda self: (cleared.append(1), clear(self))[1])
    t, model = train_file(corpus_file, case, batch_bytes=8 << 10)
    assert model.merges == exp_merges and model.vocab == exp_vocab
    check_stats(t, base, exp_merges, hh.FILE_MERGES, u16)
    assert len(cleared) == 1


# ---------------------------------------------------------------- 7. train_from across the seam
V1, V2 = 80, 300


@pytest.mark.parametrize("h", [150, 40])
def test_train_from_across_the_seam(bound, monkeypatch, corpus_file, h):
    """h = 150: a resumed u16 stage 1, then a hand-over whose replay is the model's triples plus stage 1's, then stage 2.
    h = 40: the model is past the bound already, so the job goes straight to the u32 load with the replay only."""
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    exp_vocab, exp_merges = hh.file_reference(corpus_file, V2)
    base = helpers.base_tokens(SP)
    old = exp_merges[:V1]
    model = BBPEModel(vocab={tok: i for tok, i in exp_vocab.items() if i < len(base) + sum(hh.fresh_flags(base, old))}, merges=old, special_tokens=SP)
    u16 = bound(len(base) + h)
    t = BBPETrainer(BBPETrainerConfig(vocab_size=len(base) + V2, **hh.FILE_CFG))
    out = t.train_from(model, [corpus_file])
    assert out.merges == exp_merges and out.vocab == exp_vocab
    want = check_stats(t, base, exp_merges, V2 - V1, u16, n_old=V1)
    assert (want["id16_stages"] >= 1) == (h == 150) and want["id32_replayed_merges"] == V1 + want["id16_merges"]


REUSE_SEAMS = {"abc_many": (8, 16), "abcdef_pairs": (6, 8)}  # name: (merges of the model, h of the resumed stage 1)


@pytest.mark.parametrize("straight", [False, True])
@pytest.mark.parametrize("name", list(REUSE_SEAMS))
def test_train_from_across_the_seam_with_reused_ids(bound, name, straight):
    """_run as train_from calls it (the specials of these cases would be cut out of a file's text as special tokens, so the
    words are handed over directly): the model's merges hold reused ids (n_old > 0 in _decode_tokens), stage 1 meets one
    more and repeats, stage 2 the rest; `straight`: the bound below the model, the replay alone."""
    c = hh.reuse_case(name)
    n_old, h = REUSE_SEAMS[name]
    u16 = bound(len(c["base"]) + (2 if straight else h))
    t = BBPETrainer(BBPETrainerConfig(vocab_size=c["vocab_size"], min_frequency=1, special_tokens=c["specials"]))
    old = c["merges"][:n_old]
    model = BBPEModel(vocab={tok: i for tok, i in c["vocab"].items() if i < len(c["base"]) + sum(hh.fresh_flags(c["base"], old))},
                      merges=old, special_tokens=c["specials"])
    toks, triples = t._resumable(model)
    budget = c["budget"] - n_old
    with t._context() as ctx:
        vocab, new = t._run(ctx, toks, t._host_words(c["types"], np.array(c["freqs"], dtype=np.uint64)), triples, budget)
    assert old + new == c["merges"] and vocab == c["vocab"]
    fresh = [k not in c["hits"] for k in range(c["n_steps"])]
    want = hh.expected_stages(len(c["base"]), fresh, budget, u16, n_old=n_old)
    assert hh.picked(t.last_stats) == want
    assert want["id16_stages"] == (0 if straight else 2) and want["id32_replayed_merges"] == n_old + want["id16_merges"]


# ---------------------------------------------------------------- 8. YABPE_ID_BITS=32
def test_id_bits_32_words(bound, monkeypatch):
    types, freqs, (exp_vocab, exp_merges) = hh.tie_reference("stems")
    u16 = bound(256 + 17)
    monkeypatch.setenv("YABPE_ID_BITS", "32")
    t = BBPETrainer(BBPETrainerConfig(vocab_size=256 + hh.TIE_BUDGET, min_frequency=1, special_tokens=[]))
    vocab, merges = t._merge_loop_words(types, np.array(freqs, dtype=np.uint64))
    assert merges == exp_merges and vocab == exp_vocab
    want = check_stats(t, helpers.base_tokens([]), exp_merges, hh.TIE_BUDGET, u16, mode="32")
    assert want == {"id16_merges": 0, "id16_stages": 0, "id32_merges": len(exp_merges), "id32_replayed_merges": 0}


def test_id_bits_32_file(bound, monkeypatch, corpus_file):
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    exp_vocab, exp_merges = hh.file_reference(corpus_file, **hh.FILE_CASES["gpt2_g3"])
    base = helpers.base_tokens(SP)
    u16 = bound(len(base) + hh.FILE_H)
    monkeypatch.setenv("YABPE_ID_BITS", "32")
    t, model = train_file(corpus_file, "gpt2_g3")
    assert model.merges == exp_merges and model.vocab == exp_vocab
    want = check_stats(t, base, exp_merges, hh.FILE_MERGES, u16, mode="32")
    assert want == {"id16_merges": 0, "id16_stages": 0, "id32_merges": hh.FILE_MERGES, "id32_replayed_merges": 0}
