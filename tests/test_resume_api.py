"""CPU: the host side of continuing from a trained model -- BBPETrainer.train_from refuses a model that is not resumable
(before it touches the GPU), BBPEModel.from_file_lossless, and the declarations of the new C entry points."""
from __future__ import annotations

import json
import re
from pathlib import Path

import pytest

from tests import helpers
from yet_another_bpe import _native
from yet_another_bpe.tokenizer import BBPETokenizer
from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

ROOT = Path(__file__).resolve().parent.parent
SP = ["<|endoftext|>"]


def corpus_en_1000(golden_dir) -> BBPETrainer:
    t = BBPETrainer(BBPETrainerConfig(vocab_size=1000, min_frequency=1, max_workers=1, special_tokens=SP))
    t._vocab = {bytes.fromhex(k): v for k, v in json.loads((golden_dir / "g1_corpus_en_vocab_1000.json").read_text()).items()}
    t._merges = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")[:743]
    return t


def test_from_file_lossless_round_trip(golden_dir, tmp_path):
    t = corpus_en_1000(golden_dir)
    t.save_lossless(tmp_path / "m")
    m = BBPEModel.from_file_lossless(tmp_path / "m")
    assert m.vocab == t._vocab and m.merges == t._merges and m.special_tokens == SP
    toks, (left, right, merged) = BBPETrainer(BBPETrainerConfig(special_tokens=SP))._resumable(m)
    assert {tok: i for i, tok in enumerate(toks)} == t._vocab and len(left) == len(right) == len(merged) == 743


def test_zero_budget_returns_the_model_unchanged(golden_dir, tmp_path):
    t = corpus_en_1000(golden_dir)
    model = BBPEModel(t._vocab, t._merges, SP)
    again = BBPETrainer(BBPETrainerConfig(vocab_size=1000, min_frequency=1, special_tokens=SP))  # 257 + 743 = 1000: nothing left
    out = again.train_from(model, [golden_dir / "corpus.en"])
    assert out.vocab == model.vocab and out.merges == model.merges and out.special_tokens == SP
    again.save_lossless(tmp_path / "same")
    assert BBPEModel.from_file_lossless(tmp_path / "same").merges == model.merges
    with pytest.raises(ValueError, match="At least one file"):
        again.train_from(model, [])
    with pytest.raises(FileNotFoundError):
        again.train_from(model, [tmp_path / "missing.txt"])


def test_refuses_a_lossy_reload_and_names_the_lossless_loader(golden_dir, tmp_path):
    t = corpus_en_1000(golden_dir)
    t.save(tmp_path / "m")
    lossy = BBPETokenizer.from_file(tmp_path / "m")
    assert lossy._merges != t._merges  # (merges whose left token holds a space are cut differently: SURVEY 8f-2)
    model = BBPEModel(lossy._vocab, lossy._merges, lossy.special_tokens)
    with pytest.raises(ValueError, match="from_file_lossless"):
        BBPETrainer(BBPETrainerConfig(vocab_size=2000, special_tokens=SP)).train_from(model, [golden_dir / "corpus.en"])


def test_refuses_other_special_tokens(golden_dir):
    t = corpus_en_1000(golden_dir)
    model = BBPEModel(t._vocab, t._merges, SP)
    with pytest.raises(ValueError, match="special tokens"):
        BBPETrainer(BBPETrainerConfig(vocab_size=2000)).train_from(model, [golden_dir / "corpus.en"])
    with pytest.raises(ValueError, match="special tokens"):
        BBPETrainer(BBPETrainerConfig(vocab_size=2000, special_tokens=SP)).train_from(BBPEModel(t._vocab, t._merges, []), [golden_dir / "corpus.en"])


def test_refuses_ids_that_are_not_dense(golden_dir):
    t = corpus_en_1000(golden_dir)
    vocab = dict(t._vocab)
    last = max(vocab, key=vocab.get)
    vocab[last] += 5
    with pytest.raises(ValueError, match="dense"):
        BBPETrainer(BBPETrainerConfig(vocab_size=2000, special_tokens=SP)).train_from(BBPEModel(vocab, t._merges, SP), [golden_dir / "corpus.en"])


def test_refuses_a_merge_with_an_unknown_operand(golden_dir):
    t = corpus_en_1000(golden_dir)
    merges = list(t._merges)
    merges[10], merges[700] = merges[700], merges[10]  # merge 700's operands do not exist yet at position 10
    with pytest.raises(ValueError, match="not a token"):
        BBPETrainer(BBPETrainerConfig(vocab_size=2000, special_tokens=SP)).train_from(BBPEModel(t._vocab, merges, SP), [golden_dir / "corpus.en"])
    with pytest.raises(ValueError, match="does not reproduce"):  # the right tokens under other ids
        swapped = dict(t._vocab)
        a, b = [k for k, v in swapped.items() if v in (500, 501)]
        swapped[a], swapped[b] = swapped[b], swapped[a]
        BBPETrainer(BBPETrainerConfig(vocab_size=2000, special_tokens=SP)).train_from(BBPEModel(swapped, t._merges, SP), [golden_dir / "corpus.en"])


def test_merge_triples_reuse_and_fresh_ids():
    base = helpers.base_tokens(["ab"])
    toks, (left, right, merged) = _native.merge_triples(base, [(b"a", b"b"), (b"ab", b"c"), (b"a", b"b")])
    assert toks == base + [b"abc"]
    assert merged.tolist() == [256, 257, 256] and left.tolist() == [97, 256, 97] and right.tolist() == [98, 99, 98]


def test_new_entry_points_are_declared():
    header = (ROOT / "include" / "yabpe.h").read_text()
    assert "#define YABPE_ABI_VERSION 2" in header
    for name in ("yabpe_load_words_resumed", "yabpe_resume_stats"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _native.SYMBOLS
    assert "yabpe_resume_stats_t" in header
    for f in ("n_unique", "n_long", "tokens", "segment_ms", "build_ms"):
        assert f in dict(_native.ResumeStats._fields_)
    for name in ("load_words_resumed", "load_words_resumed_ptr", "resume_stats"):
        assert hasattr(_native.Context, name)
    csrc = ROOT / "yet-another-bpe_amd" / "csrc"
    logic = (csrc / "replay_logic.h").read_text()
    assert "rp_lookup" in logic and "rp_walk_heap" in logic and "rp_walk_lanes" in logic
    kernels = (csrc / "yabpe_replay_kernels.h").read_text()
    for k in ("k_replay_words", "k_load_words_tok", "k_load_long_tok"):
        assert k in kernels
