"""GPU (-m gpu): vocabularies past 65,534 tokens through BBPETrainer / BBPETokenizer: the u16 stage, the
hand-over by replay, the u32 stage, continuing such a model, and the device encoder / decoder at ids past 65,535.  Bit-exact
against the C oracle: merges and ids."""
from __future__ import annotations

import pytest

from oracle import oracle
from tests import id32_helpers
from yet_another_bpe.tokenizer import BBPETokenizer
from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

pytestmark = pytest.mark.gpu
CFG = dict(min_frequency=1, max_workers=1, special_tokens=[])


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    path = tmp_path_factory.mktemp("id32") / "corpus.txt"
    path.write_bytes(b" ".join(id32_helpers.api_corpus_words()))
    return path


@pytest.fixture(scope="module")
def expected():
    """The oracle's model at 66,560 and at 67,000 tokens (computed once, shared), after the recipe's own check.  On the words
    as drawn the oracle gives 66,304 merges, no reused id, and the ids 65,534, 65,535 and 65,536 are operands of merges
    65,279 .. 65,281 (counted from 0).  The file's pre-tokens carry the GPT-2 space prefix (all but the first); the oracle on
    those gives 66,304 merges without a reused id as well, creates the three ids with merges 65,278 .. 65,280 and uses 65,534
    in merge 65,279 (65,535 and 65,536 stay unused there) -- both are asserted, so a changed recipe fails here, on the CPU."""
    drawn_vocab, drawn = oracle.merge_loop(list(id32_helpers.api_corpus_words()), 66_560, 1, [])
    assert len(drawn) == 66_304 and len(drawn_vocab) == 66_560
    for k, tid in enumerate((65_534, 65_535, 65_536)):
        assert tid in (drawn_vocab[drawn[65_279 + k][0]], drawn_vocab[drawn[65_279 + k][1]]), tid
    words = id32_helpers.api_expected_words()
    vocab, merges = oracle.merge_loop(words, 66_560, 1, [])
    assert len(merges) == 66_304 and len(vocab) == 66_560
    assert [vocab[l + r] for l, r in merges[65_278:65_281]] == [65_534, 65_535, 65_536]
    assert 65_534 in (vocab[merges[65_279][0]], vocab[merges[65_279][1]])
    big = oracle.merge_loop(words, 67_000, 1, [])
    assert len(big[1]) == 66_744
    return (vocab, merges), big


@pytest.fixture(scope="module")
def model_66560(corpus, expected):
    t = BBPETrainer(BBPETrainerConfig(vocab_size=66_560, **CFG))
    model = t.train([corpus])
    return t, model


def test_train_past_the_u16_bound(corpus, expected, model_66560, monkeypatch):
    (exp_vocab, exp_merges), _big = expected
    t, model = model_66560
    assert model.merges == exp_merges and model.vocab == exp_vocab
    st = t.last_stats
    assert (st["id16_merges"], st["id32_merges"], st["id32_replayed_merges"]) == (65_278, 1_026, 65_278), st
    print("stages:", {k: st[k] for k in ("id16_merges", "id16_stages", "id16_train_ms", "id32_merges", "id32_load_ms", "train_ms")})
    monkeypatch.setenv("YABPE_ID_BITS", "32")
    t32 = BBPETrainer(BBPETrainerConfig(vocab_size=66_560, **CFG))
    m32 = t32.train([corpus])
    assert m32.merges == exp_merges and m32.vocab == exp_vocab
    assert (t32.last_stats["id16_merges"], t32.last_stats["id32_merges"]) == (0, 66_304)


def test_u16_only_keeps_its_error(corpus, monkeypatch):
    from yet_another_bpe import _native

    monkeypatch.setenv("YABPE_ID_BITS", "16")
    with pytest.raises(_native.YabpeError) as e:
        BBPETrainer(BBPETrainerConfig(vocab_size=66_560, **CFG)).train([corpus])
    assert e.value.code == -4


def test_train_from_goes_straight_to_the_u32_path(corpus, expected, model_66560, tmp_path):
    _small, (big_vocab, big_merges) = expected
    t, model = model_66560
    t2 = BBPETrainer(BBPETrainerConfig(vocab_size=67_000, **CFG))
    out = t2.train_from(model, [corpus])
    assert out.merges == big_merges and out.vocab == big_vocab
    assert t2.last_stats["id16_merges"] == 0 and t2.last_stats["id16_stages"] == 0 and t2.last_stats["id32_merges"] == 440
    t.save_lossless(tmp_path / "m")
    t3 = BBPETrainer(BBPETrainerConfig(vocab_size=67_000, **CFG))
    again = t3.train_from(BBPEModel.from_file_lossless(tmp_path / "m"), [corpus])
    assert again.merges == big_merges and again.vocab == big_vocab


def test_batched_corpus_gives_the_same_model(corpus, expected):
    (exp_vocab, exp_merges), _big = expected
    model = BBPETrainer(BBPETrainerConfig(vocab_size=66_560, **CFG)).train([corpus], batch_bytes=32 << 10)
    assert model.merges == exp_merges and model.vocab == exp_vocab


def test_device_encoder_and_decoder_at_large_ids(model_66560):
    _t, model = model_66560
    tok = BBPETokenizer(vocab=model.vocab, merges=model.merges, special_tokens=[])
    words = id32_helpers.api_corpus_words()
    # 50 words of the corpus: the first 25, and 25 whose ids reach past 65,535
    late = id32_helpers.words_with_late_ids(tok, model.vocab, words, 25)
    assert len(late) == 25
    texts = [" " + w.decode() for w in [*words[:25], *late]] + ["an unseen string of words", "zzzzqqqq 123 xyzzy"]
    ids = tok.encode_batch(texts)
    assert tok.encode_batch_device(texts) == ids
    assert max(max(row) for row in ids if row) >= 65_536
    assert tok.decode_batch_device(ids) == texts == tok.decode_batch(ids)
