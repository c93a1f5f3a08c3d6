"""GPU (-m gpu): training with a maximum token length (option max_token_bytes / BBPETrainerConfig.max_token_length) against
the independent plain-Python trainer of tests/limit_helpers.py: merges and vocabulary ids, bit-exact.  Every run has
verify = 1: after the job the incremental pair table is compared with a recount under the same limit."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from tests import dist_workers, helpers, limit_dist_workers, limit_helpers as lh

pytestmark = pytest.mark.gpu
SP = lh.SP
E_INVALID = -1
BASE = 257  # 256 bytes + the special token


def gpu_train(words, freq, num_merges, min_frequency, limit, dedup=False, options=None):
    from yet_another_bpe import _native

    flat, off = helpers.flatten(words)
    opts = {"verify": 1}
    if limit is not None:
        opts["max_token_bytes"] = limit
    opts.update(options or {})
    return _native.train_words(flat, off, freq, helpers.base_tokens(SP), num_merges, min_frequency, dedup=dedup, options=opts)


def layout_args(layout, words):
    """(words, freq, dedup) of the three layouts of tests/test_gpu_parity.py"""
    if layout == "weighted":
        uw, fq = helpers.pooled(words)
        return uw, fq, False
    return list(words), None, layout == "device_dedup"


# ---------------------------------------------------------------- parity on the 6,000 pre-tokens
@pytest.mark.parametrize("layout", ["flat", "weighted", "device_dedup"])
@pytest.mark.parametrize("limit", [2, 3, 4, 6, 8, 16])
def test_parity_with_the_helper(layout, limit):
    exp_vocab, exp_merges, _trace = lh.en_model(limit)
    words, freq, dedup = layout_args(layout, lh.en_words())
    vocab, merges = gpu_train(words, freq, 400, 2, limit, dedup=dedup)
    assert merges == exp_merges
    assert vocab == exp_vocab
    assert all(len(l) + len(r) <= limit for l, r in merges)
    assert all(len(t) <= limit for t, i in vocab.items() if i >= BASE)
    if limit == 16:  # longer than anything the run creates: the run without a limit
        free_vocab, free_merges = gpu_train(words, freq, 400, 2, None, dedup=dedup)
        assert merges == free_merges and vocab == free_vocab and len(merges) == 400


def test_exhaustion_is_a_clean_stop():
    exp_vocab, exp_merges, trace = lh.en_model(3, num_merges=1 << 20, min_frequency=1)
    assert len(exp_merges) == 926 and trace["stop"] == "no_pairs"
    uw, fq = helpers.pooled(lh.en_words())
    vocab, merges = gpu_train(uw, fq, 5000, 1, 3)
    assert len(merges) == 926
    assert merges == exp_merges and vocab == exp_vocab


@pytest.mark.parametrize("options", [{"split": 0}, {"split": 1}, {"hist": 0}, {"batch_max": 1}, {"table_min_log2": 10, "check_interval": 7},
                                     {"cand_argmax": 0}], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_forced_forms_at_limit_4(options):
    exp_vocab, exp_merges, _trace = lh.en_model(4)
    vocab, merges = gpu_train(list(lh.en_words()), None, 400, 2, 4, options=options)
    assert merges == exp_merges and vocab == exp_vocab


# ---------------------------------------------------------------- long words and runs
@lru_cache(maxsize=None)
def long_corpus() -> tuple:
    short = list(lh.en_words()[:400])
    long = [b"a" * 200, b"a" * 201, b"ab" * 100, b"a" * 64, b"ab" * 32 + b"a", b"abc" * 100, b"the " * 60, b" " * 300, b"xyxyx" * 13 + b"aaa" * 40]
    assert all(64 <= len(w) <= 300 for w in long)
    return tuple(short + long + long[:3])


@pytest.mark.parametrize("layout", ["flat", "weighted"])
@pytest.mark.parametrize("limit", [3, 4])
def test_long_words_and_runs(layout, limit):
    uw, fq = helpers.pooled(long_corpus())
    exp_vocab, exp_merges = lh.train(uw, fq, 600, 1, SP, limit=limit)
    words, freq, dedup = layout_args(layout, long_corpus())
    vocab, merges = gpu_train(words, freq, 600, 1, limit, dedup=dedup)
    assert merges == exp_merges and vocab == exp_vocab
    assert all(len(l) + len(r) <= limit for l, r in merges)


def test_a_run_of_one_byte_at_limit_4():
    vocab, merges = gpu_train([b"a" * 200], None, 50, 1, 4)
    assert merges == [(b"a", b"a"), (b"aa", b"aa")]
    assert vocab[b"aa"] == BASE and vocab[b"aaaa"] == BASE + 1 and len(vocab) == BASE + 2
    assert lh.train([b"a" * 200], None, 50, 1, SP, limit=4)[1] == merges


# ---------------------------------------------------------------- the limit belongs to the load
def test_continue_equals_one_shot():
    """Two yabpe_train calls on one load: the limit read at the load holds for both."""
    from yet_another_bpe import _native
    from yet_another_bpe.trainer import BBPETrainer

    exp_vocab, exp_merges, _trace = lh.en_model(4)
    uw, fq = helpers.pooled(lh.en_words())
    flat, off = helpers.flatten(uw)
    base = helpers.base_tokens(SP)
    with _native.Context() as ctx:
        ctx.set_option("verify", 1)
        ctx.set_option("max_token_bytes", 4)
        ctx.set_vocab(base)
        ctx.load_words(flat, off, fq)
        ctx.set_option("max_token_bytes", 0)  # (too late for this load: it is not read again)
        l0, r0, m0, _c = ctx.train(150, 2)
        l1, r1, m1, _c = ctx.train(250, 2)
        assert ctx.verify_table() == 0
    assert len(l0) == 150 and len(l1) == 250
    vocab, merges = BBPETrainer._decode_merges(base, np.concatenate([l0, l1]), np.concatenate([r0, r1]), np.concatenate([m0, m1]))
    assert merges == exp_merges and vocab == exp_vocab


def test_refusals():
    from yet_another_bpe import _native
    from yet_another_bpe.trainer import BBPETrainer

    uw, fq = helpers.pooled(lh.en_words()[:500])
    flat, off = helpers.flatten(uw)
    base = helpers.base_tokens(SP)
    with _native.Context() as ctx:
        ctx.set_option("verify", 1)
        ctx.set_vocab(base)
        for bad in (1, -1, -8):
            ctx.set_option("max_token_bytes", bad)
            with pytest.raises(_native.YabpeError, match="max_token_bytes") as e:
                ctx.load_words(flat, off, fq)
            assert e.value.code == E_INVALID
        ctx.set_option("max_token_bytes", 0)  # the context is still usable
        ctx.load_words(flat, off, fq)
        left, right, merged, _c = ctx.train(50, 2)
        assert ctx.verify_table() == 0
    assert BBPETrainer._decode_merges(base, left, right, merged)[1] == lh.train(uw, fq, 50, 2, SP)[1]  # 0 = no limit


# ---------------------------------------------------------------- through the trainer: text in, model out
@lru_cache(maxsize=None)
def en_file_model(limit, num_merges, start=()):
    uw, fq = helpers.pooled(helpers.corpus_en_words())
    return lh.train(uw, fq, num_merges, 2, SP, limit=limit, start_merges=start)


def _config(vocab_size, limit):
    from yet_another_bpe.trainer import BBPETrainerConfig

    return BBPETrainerConfig(vocab_size=vocab_size, min_frequency=2, special_tokens=SP, max_token_length=limit)


def test_text_in_model_out(golden_dir, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer

    monkeypatch.setenv("YABPE_OPT_verify", "1")
    exp_vocab, exp_merges = en_file_model(4, 300)
    assert len(exp_merges) == 300
    files = [golden_dir / "corpus.en"]
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    host = BBPETrainer(_config(BASE + 300, 4)).train(files)
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    dev = BBPETrainer(_config(BASE + 300, 4)).train(files)
    batched = BBPETrainer(_config(BASE + 300, 4)).train(files, batch_bytes=32768)
    for got in (host, dev, batched):
        assert got.merges == exp_merges and got.vocab == exp_vocab
        assert all(len(l) + len(r) <= 4 for l, r in got.merges)


@pytest.mark.parametrize("batch_bytes", [None, 32768])
def test_resume_under_the_same_limit(golden_dir, tmp_path, monkeypatch, batch_bytes):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer

    monkeypatch.setenv("YABPE_OPT_verify", "1")
    if batch_bytes:
        monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    files = [golden_dir / "corpus.en"]
    exp_vocab, exp_merges = en_file_model(4, 400)
    first = BBPETrainer(_config(BASE + 150, 4))
    part = first.train(files)
    assert part.merges == exp_merges[:150]
    first.save_lossless(tmp_path / "v1")
    out = BBPETrainer(_config(BASE + 400, 4)).train_from(BBPEModel.from_file_lossless(tmp_path / "v1"), files, batch_bytes=batch_bytes)
    scratch = BBPETrainer(_config(BASE + 400, 4)).train(files)
    assert out.merges == scratch.merges == exp_merges
    assert out.vocab == scratch.vocab == exp_vocab


def test_resume_with_a_smaller_limit_constrains_only_the_new_merges(golden_dir, tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer

    monkeypatch.setenv("YABPE_OPT_verify", "1")
    files = [golden_dir / "corpus.en"]
    first = BBPETrainer(_config(BASE + 150, None))
    part = first.train(files)
    assert len(part.merges) == 150 and max(len(l) + len(r) for l, r in part.merges) > 3  # replayed merges longer than the new limit
    first.save_lossless(tmp_path / "free")
    out = BBPETrainer(_config(BASE + 400, 3)).train_from(BBPEModel.from_file_lossless(tmp_path / "free"), files)
    exp_vocab, exp_new = en_file_model(3, 250, start=tuple(part.merges))
    assert out.merges[:150] == part.merges
    assert out.merges[150:] == exp_new and out.vocab == exp_vocab
    assert all(len(l) + len(r) <= 3 for l, r in out.merges[150:])


# ---------------------------------------------------------------- two ranks, one GPU
def test_two_ranks_one_gpu_at_limit_4():
    _vocab, exp_merges, _trace = lh.en_model(4)
    outs = dist_workers.spawn(limit_dist_workers.gpu_sharded_limit, 2, 4, 400, 2, timeout=600)
    for merges, n_words in outs:
        assert [(bytes.fromhex(a), bytes.fromhex(b)) for a, b in merges] == exp_merges
    assert outs[0][1] > 0 and outs[1][1] > 0  # both ranks held words
