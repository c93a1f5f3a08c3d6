"""CPU: how BBPETrainer chooses the id width: the stage arithmetic of _run with a stub context in place of
the device, YABPE_ID_BITS, and the sharded drivers' refusal of a budget past 65,534."""
from __future__ import annotations

import numpy as np
import pytest

from yet_another_bpe import distributed, trainer
from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig


def fresh_pair(j: int) -> tuple[int, int]:
    """The operands of the j-th fresh token of the stub's model (id 256 + j): every byte pair first, then two-byte token + byte"""
    return (j >> 8, j & 255) if j < 65_536 else (256 + ((j - 65_536) >> 8), (j - 65_536) & 255)


class StubContext:
    """Plays a scripted merge loop: merge k of the job makes the next fresh token (fresh_pair), or repeats the last fresh merge
    where the script says the merge reuses an id; the job has `available` merges before a stop rule ends it."""
    log: list = []

    def __init__(self, script):
        self.script, self.id_bits, self.n_tokens, self.done = script, 16, 0, 0

    def set_option(self, name, value):
        if name == "id_bits":
            self.id_bits = value

    def set_vocab(self, toks):
        self.n_tokens = len(toks)
        StubContext.log.append(("set_vocab", self.id_bits, len(toks)))

    def _load(self, kind, triples):
        self.done = 0 if triples is None else len(triples[0])
        StubContext.log.append((kind, self.id_bits, self.done))

    def load_words(self, flat, off, freq=None, dedup=False):
        self._load("load", None)

    def load_words_resumed(self, flat, off, freq, triples, dedup=False):
        self._load("load_resumed", triples)

    def train(self, num_merges, min_frequency):
        StubContext.log.append(("train", self.id_bits, num_merges))
        if self.id_bits == 16:
            assert self.n_tokens + num_merges <= 65_534 or num_merges <= self.script.get("u16_may_ask", 0)
        left, right, merged = [], [], []
        for _ in range(num_merges):
            if self.done >= self.script["available"]:
                break
            j = self.n_tokens - 256  # fresh tokens so far
            if self.done in self.script.get("reused", ()):
                l, r = fresh_pair(j - 1)  # the last fresh merge again: its bytes are a token already
                m = self.n_tokens - 1
            else:
                l, r = fresh_pair(j)
                m = self.n_tokens
                self.n_tokens += 1
            left.append(l), right.append(r), merged.append(m)
            self.done += 1
        u32 = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
        return u32(left), u32(right), u32(merged), np.ones(len(merged), dtype=np.uint64)

    def stats(self):
        return {"train_ms": 1.0, "merges_done": self.done}

    def resume_stats(self):
        return {"segment_ms": 2.0, "build_ms": 3.0}

    def pool_clear(self):
        StubContext.log.append(("pool_clear",))

    def close(self):
        StubContext.log.append(("close", self.id_bits))


def run(monkeypatch, vocab_size, script, toks=None, triples=None, mode=None):
    if mode is None:
        monkeypatch.delenv("YABPE_ID_BITS", raising=False)
    else:
        monkeypatch.setenv("YABPE_ID_BITS", mode)
    StubContext.log = []
    t = BBPETrainer(BBPETrainerConfig(vocab_size=vocab_size, min_frequency=1, special_tokens=[]))
    monkeypatch.setattr(t, "_context", lambda: StubContext(script))
    toks = toks or [bytes([b]) for b in range(256)]
    words = (np.zeros(2, np.uint8), np.array([0, 2], np.uint64), None)
    n_old = 0 if triples is None else len(triples[0])
    vocab, merges = t._run(StubContext(script), toks, words, triples, vocab_size - 256 - n_old)
    return t.last_stats, StubContext.log, merges


def test_stage_arithmetic():
    assert trainer.stage1_merges(256, 66_304) == 65_278
    assert trainer.stage1_merges(256, 100) == 100
    assert trainer.stage1_merges(65_534, 10) == 0 and trainer.stage1_merges(70_000, 10) == 0
    assert trainer.stage1_merges(65_530, 0) == 0


def test_a_budget_inside_the_u16_space_takes_the_old_route(monkeypatch):
    st, log, merges = run(monkeypatch, 65_534, {"available": 10 ** 9})
    assert log == [("set_vocab", 16, 256), ("load", 16, 0), ("train", 16, 65_278)] and len(merges) == 65_278
    assert "id32_merges" not in st


def test_two_stages(monkeypatch):
    st, log, merges = run(monkeypatch, 66_560, {"available": 10 ** 9})
    assert [e for e in log if e[0] == "train"] == [("train", 16, 65_278), ("train", 32, 1_026)]
    assert ("load_resumed", 32, 65_278) in log and ("set_vocab", 32, 65_534) in log and log[-1] == ("close", 32)
    assert (st["id16_merges"], st["id16_stages"], st["id32_merges"], st["id32_replayed_merges"], st["id32_load_ms"]) == (65_278, 1, 1_026, 65_278, 5.0)
    assert len(merges) == 66_304


def test_stage_one_repeats_after_reused_ids(monkeypatch):
    st, log, merges = run(monkeypatch, 66_560, {"available": 10 ** 9, "reused": {10, 20, 65_279}})
    # the first call leaves 2 ids (two merges reused one), the second leaves 1 (one more reuse), the third none
    assert [e for e in log if e[0] == "train"] == [("train", 16, 65_278), ("train", 16, 2), ("train", 16, 1), ("train", 32, 1_023)]
    assert (st["id16_merges"], st["id16_stages"], st["id32_merges"]) == (65_281, 3, 1_023)
    assert len(merges) == 66_304


def test_a_stop_inside_stage_one_ends_the_job(monkeypatch):
    st, log, merges = run(monkeypatch, 100_000, {"available": 300})
    assert [e for e in log if e[0] == "train"] == [("train", 16, 65_278)] and len(merges) == 300
    assert (st["id16_merges"], st["id32_merges"]) == (300, 0) and not any(e[1] == 32 for e in log if len(e) > 1)


def test_a_model_past_the_bound_goes_straight_to_stage_two(monkeypatch):
    n_old = 65_534 - 256
    pairs = [fresh_pair(j) for j in range(n_old)]
    toks = [bytes([b]) for b in range(256)] + [bytes(p) for p in pairs]
    triples = (np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32),
               np.arange(256, 65_534, dtype=np.uint32))
    st, log, merges = run(monkeypatch, 66_000, {"available": 10 ** 9}, toks=toks, triples=triples)
    assert log == [("set_vocab", 32, 65_534), ("load_resumed", 32, n_old), ("train", 32, 466)]
    assert (st["id16_merges"], st["id16_stages"], st["id32_merges"]) == (0, 0, 466) and len(merges) == 466


def test_id_bits_environment(monkeypatch):
    for value, want in (("16", "16"), ("32", "32"), ("auto", "auto"), ("", "auto"), (" AUTO ", "auto")):
        monkeypatch.setenv("YABPE_ID_BITS", value)
        assert trainer.id_bits_mode() == want
    monkeypatch.delenv("YABPE_ID_BITS")
    assert trainer.id_bits_mode() == "auto"
    for bad in ("24", "u32", "wide"):
        monkeypatch.setenv("YABPE_ID_BITS", bad)
        with pytest.raises(ValueError, match="YABPE_ID_BITS"):
            trainer.id_bits_mode()
    st, log, merges = run(monkeypatch, 300, {"available": 10 ** 9}, mode="32")
    assert log == [("set_vocab", 32, 256), ("load", 32, 0), ("train", 32, 44)] and st["id32_merges"] == 44
    st, log, merges = run(monkeypatch, 66_560, {"available": 10 ** 9, "u16_may_ask": 66_304}, mode="16")
    assert log == [("set_vocab", 16, 256), ("load", 16, 0), ("train", 16, 66_304)]


def test_sharded_drivers_name_the_limit():
    cfg = BBPETrainerConfig(vocab_size=65_535, min_frequency=1, special_tokens=[])
    with pytest.raises(ValueError, match="65,534"):
        distributed.train_text_sharded(None, ["nowhere.txt"], cfg, 0, 1)
    with pytest.raises(ValueError, match="65,534"):
        distributed.train_device_text_sharded(None, None, cfg, 0, 1)
    trainer.check_sharded_budget(65_534)
