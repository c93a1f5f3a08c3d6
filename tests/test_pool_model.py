"""CPU: the rules the word-pool kernels share with their CPU model (yet-another-bpe_amd/csrc/pool_logic.h: masked hash, home
and next slot, match, growth) run by tests/hostmodel/pool_model.cpp in the kernels' shape -- probe every call-unique word,
then grow, then append every new one -- over sequences of adds, against collections.Counter.  Also the trainer's grouping of
chunks into batches (a plain function)."""
from __future__ import annotations

import ctypes
import random
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from tests import helpers

HM = Path(__file__).resolve().parent / "hostmodel"
SPLITS = (1, 2, 7, 64)
HASH_BITS = (64, 4, 0)


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libpool_model.so", HM / "pool_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "pool_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.pool_model_new.restype = ctypes.c_void_p
    lib.pool_model_new.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.pool_model_free.argtypes = [ctypes.c_void_p]
    lib.pool_model_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    lib.pool_model_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.pool_model_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.pool_model_check.argtypes = [ctypes.c_void_p]
    return lib


class ModelPool:
    def __init__(self, lib, init_slots=2, init_bytes=1, hash_bits=64):
        self.lib, self.h = lib, lib.pool_model_new(init_slots, init_bytes, hash_bits)

    def add(self, words, freq=None):
        flat, off = helpers.flatten(words)
        flat = np.append(flat, np.uint8(0))  # (never an empty buffer)
        fq = None if freq is None else np.ascontiguousarray(freq, dtype=np.uint64)
        assert self.lib.pool_model_add(self.h, flat.ctypes.data, off.ctypes.data, fq.ctypes.data if fq is not None and len(fq) else None,
                                       len(words)) == 0
        assert self.lib.pool_model_check(self.h) == 0

    def stats(self):
        out = np.zeros(8, np.uint64)
        self.lib.pool_model_stats(self.h, out.ctypes.data)
        return dict(zip(("n_unique", "n_bytes", "slot_capacity", "arena_capacity", "slot_growths", "arena_growths", "dropped", "probe_steps"),
                        out.tolist()))

    def items(self):
        st = self.stats()
        blob, off, cnt = np.zeros(st["n_bytes"] + 1, np.uint8), np.zeros(st["n_unique"] + 1, np.uint64), np.zeros(st["n_unique"] + 1, np.uint64)
        self.lib.pool_model_get(self.h, blob.ctypes.data, off.ctypes.data, cnt.ctypes.data)
        b, o = blob.tobytes(), off.tolist()
        assert o[0] == 0 and o[-1] == st["n_bytes"]
        pairs = [(b[o[i]:o[i + 1]], int(cnt[i])) for i in range(st["n_unique"])]
        assert len({w for w, _ in pairs}) == len(pairs)  # every byte string once
        return dict(pairs)

    def close(self):
        self.lib.pool_model_free(self.h)


def split_calls(words, k):
    """k consecutive pieces, with an empty call after the first one"""
    cuts = [len(words) * i // k for i in range(k + 1)]
    calls = [words[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return calls[:1] + [[]] + calls[1:]


def word_lists():
    rng = random.Random(7)
    few = [bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 4))) for _ in range(3000)]            # many repeats, empties
    wide = [bytes(rng.randrange(256) for _ in range(rng.choice((1, 2, 3, 63, 64, 65, 130)))) for _ in range(600)]
    wide += wide[::3] + [b"", b"\x00", b"\x00\x00", b"\xff", b"\xff\x00"]
    return {"abc": few, "bytes": wide}


@pytest.mark.parametrize("bits", HASH_BITS)
@pytest.mark.parametrize("name", ["abc", "bytes"])
def test_sequences_of_adds_equal_counter(model, name, bits):
    words = word_lists()[name]
    exp = Counter(w for w in words if w)
    for k in SPLITS:
        p = ModelPool(model, 2, 1, bits)  # 2 slots, 1 byte: every add that brings a new word grows something
        for call in split_calls(words, k):
            p.add(call)
        st = p.stats()
        assert p.items() == dict(exp), (name, bits, k)
        assert st["n_unique"] == len(exp) and st["n_bytes"] == sum(len(w) for w in exp)
        assert st["dropped"] == sum(1 for w in words if not w)
        assert st["slot_growths"] >= 1 and st["arena_growths"] >= 1
        assert st["slot_capacity"] >= 2 * st["n_unique"] and st["slot_capacity"] & (st["slot_capacity"] - 1) == 0
        p.close()


def test_weighted_adds_and_counts_past_2_32(model):
    words = [b"a", b"bb", b"a", b"", b"ccc"]
    p = ModelPool(model)
    p.add(words, [5, 7, 11, 13, 1 << 31])
    p.add(words, [5, 7, 11, 13, 1 << 31])
    p.add([b"ccc"], [1 << 31])
    assert p.items() == {b"a": 32, b"bb": 14, b"ccc": 3 << 31}
    assert p.stats()["dropped"] == 26
    p.close()


def test_one_chain_probes_linearly_and_more_bits_probe_less(model):
    words = [bytes([65 + i % 26, 65 + i // 26]) for i in range(400)]
    steps = {}
    for bits in HASH_BITS:
        p = ModelPool(model, 1024, 4096, bits)
        p.add(words)
        p.add(words)  # the find path: every word walks its chain to its own entry
        assert p.items() == dict(Counter(words + words))
        steps[bits] = p.stats()["probe_steps"]
        p.close()
    assert steps[0] >= 400 * 401 // 2  # one chain: word i of the second add passes i entries
    assert steps[64] < steps[4] < steps[0]


def test_growth_rule_and_masked_hash(model):
    # (the header's functions through a tiny pool: capacities double until they hold what is asked)
    p = ModelPool(model, 2, 1)
    p.add([b"abcdefgh" * 3])  # 24 bytes into a 1-byte arena: 1 -> 32
    st = p.stats()
    assert st["arena_capacity"] == 32 and st["slot_capacity"] == 2 and st["slot_growths"] == 0
    p.add([b"x", b"y"])  # 3 words: 2 * 3 > 2 -> 8 slots
    st = p.stats()
    assert st["slot_capacity"] == 8 and st["slot_growths"] == 1 and st["arena_capacity"] == 32
    p.close()
    p = ModelPool(model, 1000, 0)  # options are rounded: a power of two of slots, at least one byte
    assert p.stats()["slot_capacity"] == 1024 and p.stats()["arena_capacity"] == 1
    p.close()


# ---------------------------------------------------------------- the trainer's batches of chunks
def test_group_chunks():
    from yet_another_bpe.trainer import group_chunks

    assert group_chunks([], 10) == []
    assert group_chunks([5], 10) == [(0, 1)]
    assert group_chunks([5, 5], 10) == [(0, 2)]
    assert group_chunks([5, 6], 10) == [(0, 1), (1, 2)]
    assert group_chunks([4, 4, 4, 4, 4], 8) == [(0, 2), (2, 4), (4, 5)]
    assert group_chunks([30, 1, 1, 30, 9, 1, 1], 10) == [(0, 1), (1, 3), (3, 4), (4, 6), (6, 7)]  # a chunk above the limit stands alone
    assert group_chunks([1] * 7, 1 << 30) == [(0, 7)]
    assert group_chunks([3, 3, 3], 1) == [(0, 1), (1, 2), (2, 3)]
    rng = random.Random(3)
    for _ in range(200):
        sizes = [rng.randint(1, 40) for _ in range(rng.randint(0, 30))]
        limit = rng.randint(1, 60)
        got = group_chunks(sizes, limit)
        assert [i for a, b in got for i in range(a, b)] == list(range(len(sizes)))  # every chunk once, in order
        for a, b in got:
            assert b > a and (sum(sizes[a:b]) <= limit or b == a + 1)
        for (a, b), (_b, c) in zip(got[:-1], got[1:]):
            assert sum(sizes[a:b]) + sizes[b] > limit  # no batch could have taken the next chunk
    with pytest.raises(ValueError):
        group_chunks([1], 0)


def test_trainer_rejects_bad_batch_arguments(tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    f = tmp_path / "t.txt"
    f.write_text("some text")
    t = BBPETrainer(BBPETrainerConfig(vocab_size=300))
    with pytest.raises(ValueError, match="positive"):
        t.train([f], batch_bytes=0)
    monkeypatch.setenv("YABPE_LAYOUT", "flat")
    with pytest.raises(ValueError, match="flat"):
        t.train([f], batch_bytes=4096)
    monkeypatch.delenv("YABPE_LAYOUT")
    monkeypatch.setenv("YABPE_PRETOKENIZE", "host")
    with pytest.raises(ValueError, match="device pre-tokeniser"):
        t.train([f], batch_bytes=4096)
