"""GPU: the persistent word pool (yabpe_pool_add / yabpe_pool_get / yabpe_pool_clear / yabpe_pool_stats) against
collections.Counter over sequences of adds -- splits, weights, device and host pointers, growth from tiny capacities, forced
hash collisions, word shapes on both sides of the wave-per-word threshold, counts past 2^32, clear and reuse, failed calls --
then training from the pool through the ABI against the reference-made golden merges, and BBPETrainer.train / train_from with
batch_bytes against the unbatched path."""
from __future__ import annotations

import random
from collections import Counter

import numpy as np
import pytest

from tests import helpers
from tests import resume_helpers as rh

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]


@pytest.fixture(scope="module")
def words():
    return helpers.corpus_en_words()


@pytest.fixture(scope="module")
def expected(words):
    return dict(Counter(words))


def new_ctx(**options):
    from yet_another_bpe import _native

    ctx = _native.Context()
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def add(ctx, ws, freq=None):
    flat, off = helpers.flatten(ws)
    ctx.pool_add(flat, off, freq)


def split_calls(ws, k):
    """k consecutive pieces, with an empty call after the first one"""
    cuts = [len(ws) * i // k for i in range(k + 1)]
    calls = [ws[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return calls[:1] + [[]] + calls[1:]


def check(ctx, exp, n_calls=None, n_words=None, dropped=0):
    """the pool equals `exp` {bytes: count}, every byte string once, and the counters add up"""
    items, st = ctx.pool_items(), ctx.pool_stats()
    assert items == exp
    assert st["n_unique"] == len(exp) == ctx.pool_get()[3]
    assert st["n_bytes"] == sum(len(w) for w in exp) == ctx.pool_get()[4]
    assert st["n_empty_dropped"] == dropped
    assert st["slot_capacity"] >= 2 * st["n_unique"] and st["slot_capacity"] & (st["slot_capacity"] - 1) == 0
    assert st["arena_capacity"] >= st["n_bytes"]
    if n_calls is not None:
        assert st["n_calls"] == n_calls
    if n_words is not None:
        assert st["n_words_added"] == n_words
    return st


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_splits(words, expected, k):
    with new_ctx() as ctx:
        assert ctx.pool_get()[3] == 0 and ctx.pool_items() == {}  # before any add
        for call in split_calls(words, k):
            add(ctx, call)
        st = check(ctx, expected, n_calls=k + 1, n_words=len(words))
        assert st["total_ms"] > 0 and st["pool_ms"] > 0 and st["probe_ms"] > 0 and st["append_ms"] > 0


def test_weighted_adds(words, expected):
    uniq, freq = helpers.pooled(words)
    with new_ctx() as ctx:
        add(ctx, uniq, freq)
        n1 = check(ctx, expected)["n_unique"]
        add(ctx, uniq, freq)
        check(ctx, {w: 2 * c for w, c in expected.items()}, n_calls=2, n_words=2 * len(uniq))
        assert ctx.pool_stats()["n_unique"] == n1
        # an offsets pointer into the middle of a larger array
        flat, off = helpers.flatten(uniq)
        ctx.pool_add(flat, off[len(uniq) // 3:], freq[len(uniq) // 3:])
        check(ctx, {w: (3 if i >= len(uniq) // 3 else 2) * expected[w] for i, w in enumerate(uniq)})


def test_device_and_host_pointers(golden_dir, words, expected):
    text = (golden_dir / "corpus.en").read_bytes()
    with new_ctx() as dev, new_ctx() as host:
        dt, do, nw = dev.pretokenize(text, special_tokens=SP)
        assert nw == len(words)
        dev.pool_add_ptr(dt, do, nw)
        dev.pretokenize_free()
        add(host, words)
        check(dev, expected, n_calls=1, n_words=len(words))
        assert dev.pool_items() == host.pool_items()


def test_growth_from_tiny_capacities(words, expected):
    with new_ctx(pool_init_slots=16, pool_init_bytes=64) as ctx:
        assert ctx.pool_get()[3] == 0
        st = ctx.pool_stats()
        assert st["slot_capacity"] == 16 and st["arena_capacity"] == 64
        for call in split_calls(words, 7):
            add(ctx, call)
        st = check(ctx, expected)
        assert st["slot_growths"] > 1 and st["arena_growths"] > 1


@pytest.mark.parametrize("bits", [4, 0])
def test_collisions(words, expected, bits):
    with new_ctx(pool_hash_bits=bits, pool_init_slots=16) as ctx:
        for call in split_calls(words, 7):
            add(ctx, call)
        check(ctx, expected)


def test_word_shapes():
    rng = random.Random(11)

    def rnd(n):
        return bytes(rng.randrange(1, 255) for _ in range(n))

    base = {n: rnd(n) for n in (1, 2, 63, 64, 65, 300, 70_000)}
    shapes = list(base.values())
    for n in (2, 64, 65, 300, 70_000):  # equal but for the last byte / the first byte; a prefix of another
        w = base[n]
        shapes += [w[:-1] + bytes([w[-1] ^ 1]), bytes([w[0] ^ 1]) + w[1:], w[:-1], w + b"z"]
    shapes += [b"\x00", b"\x00\x00", b"\xff", b"\xff\xff", b"a\x00b", b"a\x00", b"\x00" * 64, b"\x00" * 65, b"\xff" * 65, b"\xff" * 300]
    assert len(set(shapes)) == len(shapes)
    first = shapes[::2] + [b"", b""] + shapes[::4]
    second = shapes + [b""] + shapes[1::2]
    third = list(reversed(shapes)) + [w + b"!" for w in shapes[:9]] + [b""]
    for bits in (64, 0):
        with new_ctx(pool_init_slots=16, pool_init_bytes=64, pool_hash_bits=bits) as ctx:
            exp: Counter = Counter()
            for n, call in enumerate((first, second, third)):  # new words, then found and new ones mixed
                rng.shuffle(call)
                add(ctx, call)
                exp.update(w for w in call if w)
                check(ctx, dict(exp), n_calls=n + 1, dropped=sum(c.count(b"") for c in (first, second, third)[:n + 1]))


def test_counts_past_2_32():
    with new_ctx() as ctx:
        for _ in range(3):
            add(ctx, [b"the", b"a"], np.array([1 << 31, 1], dtype=np.uint64))
        check(ctx, {b"the": 3 << 31, b"a": 3})


def test_clear_and_reuse(words, expected):
    half = len(words) // 2
    with new_ctx() as ctx:
        add(ctx, words[:half])
        ctx.pool_clear()
        assert ctx.pool_get()[3] == 0 and ctx.pool_items() == {} and ctx.pool_stats()["n_calls"] == 0
        add(ctx, words[:half])
        # an unrelated corpus loaded (and trained) between two adds leaves the pool alone, and the pool leaves it alone
        ctx.set_vocab(helpers.base_tokens(SP))
        other = [b"hello", b"help", b"hello", b"shell"]
        ctx.load_words(*helpers.flatten(other), dedup=True)
        check(ctx, dict(Counter(words[:half])))
        add(ctx, words[half:])
        left, _right, _merged, count = ctx.train(3, 1)
        assert len(left) == 3 and int(count[0]) == 4 and ctx.verify_table() == 0  # (h, e) / (e, l): 4 occurrences each
        check(ctx, expected, n_calls=2, n_words=len(words))
        ctx.pool_clear()
        assert ctx.stats()["n_words"] == 3  # the corpus is still there


def test_failed_call_leaves_the_pool_as_it_was(words):
    from yet_another_bpe import _native

    some = words[:500]
    flat, off = helpers.flatten(some)
    with new_ctx() as ctx:
        add(ctx, some)
        before, st0 = ctx.pool_items(), ctx.pool_stats()
        with pytest.raises(_native.YabpeError) as e:
            ctx.pool_add_ptr(flat.ctypes.data, 0, len(some))  # word_off == NULL
        assert e.value.code == -1
        with pytest.raises(_native.YabpeError) as e:
            ctx.pool_add_ptr(flat.ctypes.data, off.ctypes.data, (1 << 32) - 2)  # over the word limit: refused before anything is read
        assert e.value.code == _native.E_CAPACITY
        with pytest.raises(_native.YabpeError) as e:
            ctx.pool_add_ptr(0, off.ctypes.data, len(some))  # bytes == NULL while the words have bytes
        assert e.value.code == -1
        st1 = ctx.pool_stats()
        assert ctx.pool_items() == before
        assert all(st1[k] == st0[k] for k in ("n_calls", "n_words_added", "n_unique", "n_bytes", "slot_growths", "arena_growths"))


def test_training_parity_through_the_abi(golden_dir, words):
    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")[:743]
    base = helpers.base_tokens(SP)
    with new_ctx() as ctx:
        for call in split_calls(words, 5)[:1] + split_calls(words, 5)[2:]:
            add(ctx, call)
        assert ctx.pool_stats()["n_calls"] == 5
        pb, po, pf, nu, _nb = ctx.pool_get()
        ctx.set_vocab(base)
        ctx.load_words_ptr(pb, po, nu, freq_ptr=pf, dedup=False)
        ctx.pool_clear()  # the load copied what it needs
        left, right, merged, _count = ctx.train(1000 - len(base), 1)
        assert ctx.verify_table() == 0
        st = ctx.stats()
        assert st["n_words"] == st["n_words_input"] == nu == len(set(words))
    toks = list(base)
    merges = []
    for l, r, m in zip(left.tolist(), right.tolist(), merged.tolist()):
        merges.append((toks[l], toks[r]))
        if m == len(toks):
            toks.append(toks[l] + toks[r])
    assert merges == g1


# ---------------------------------------------------------------- the trainer
def config(**kw):
    from yet_another_bpe.trainer import BBPETrainerConfig

    return BBPETrainerConfig(**{"vocab_size": 1000, "min_frequency": 1, "special_tokens": SP, "chunk_size_bytes": 4096, **kw})


def test_trainer_batched_equals_unbatched(golden_dir, monkeypatch):
    """The golden merges were made with the corpus as ONE chunk; cut into 4096-byte chunks the same text gives other
    pre-tokens at the cuts (28,796 instead of 28,772) and other merges from the 103rd on.  So: at 4096-byte chunks the batched
    path must equal the unbatched one AND the oracle on the host pre-tokeniser's words for that chunking; with one chunk it
    must equal the golden merges."""
    from oracle import oracle
    from yet_another_bpe.trainer import BBPETrainer

    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")[:743]
    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    monkeypatch.delenv("YABPE_BATCH_BYTES", raising=False)
    files = [golden_dir / "corpus.en"]
    t0 = BBPETrainer(config())
    cut_words = [bytes(s) for s in t0._preprocess_corpus(files)]
    exp_vocab, exp_merges = oracle.train_flat(*helpers.flatten(cut_words), 1000, 1, SP)
    plain = t0.train(files)
    assert t0.last_stats["n_words_input"] == len(cut_words)  # every occurrence went into one load
    assert plain.merges == exp_merges and plain.vocab == exp_vocab
    for b in (4096, 10_000, 1 << 30):
        t = BBPETrainer(config())
        got = t.train(files, batch_bytes=b)
        assert got.merges == plain.merges and got.vocab == plain.vocab, b
        assert t.last_stats["n_words_input"] == t.last_stats["n_words"] == len(set(cut_words))  # loaded from the pool
    # the environment variable does what the argument does
    monkeypatch.setenv("YABPE_BATCH_BYTES", "10000")
    t = BBPETrainer(config())
    got = t.train(files)
    assert got.merges == plain.merges and got.vocab == plain.vocab
    assert t.last_stats["n_words_input"] == len(set(cut_words))
    # one chunk: the reference-made golden merges
    assert BBPETrainer(config(chunk_size_bytes=1 << 30)).train(files).merges == g1


def test_trainer_several_files_errors_and_layout(golden_dir, tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPETrainer

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    monkeypatch.delenv("YABPE_BATCH_BYTES", raising=False)
    files = [golden_dir / "data/sample.txt", golden_dir / "data/empty.txt", golden_dir / "data/unicode.txt", golden_dir / "data/multiline.txt"]
    cfg = dict(vocab_size=300, special_tokens=["[PAD]", "[UNK]"], chunk_size_bytes=64)
    plain = BBPETrainer(config(**cfg)).train(files)
    for b in (64, 200, 1 << 20):  # (chunks of different files share a batch)
        got = BBPETrainer(config(**cfg)).train(files, batch_bytes=b)
        assert got.merges == plain.merges and got.vocab == plain.vocab, b
    only_empty = BBPETrainer(config(**cfg)).train([golden_dir / "data/empty.txt"], batch_bytes=64)
    assert only_empty.merges == [] and len(only_empty.vocab) == 258
    # an invalid byte in the second batch: the reference's message with the position in the file
    bad = tmp_path / "bad.txt"
    bad.write_bytes(b"fine text " * 600 + b"\xff\xfe oops")
    with pytest.raises(ValueError, match=r"bad\.txt contains invalid UTF-8 at position 6000\."):
        BBPETrainer(config()).train([golden_dir / "data/sample.txt", bad], batch_bytes=4096)
    with pytest.raises(FileNotFoundError):
        BBPETrainer(config()).train([tmp_path / "missing.txt"], batch_bytes=4096)
    monkeypatch.setenv("YABPE_LAYOUT", "flat")
    with pytest.raises(ValueError, match="flat"):
        BBPETrainer(config()).train(files, batch_bytes=4096)


def test_train_from_batched_equals_unbatched(golden_dir, tmp_path, monkeypatch):
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    monkeypatch.delenv("YABPE_BATCH_BYTES", raising=False)
    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")[:743]
    files = [golden_dir / "corpus.en"]
    first = BBPETrainer(config(vocab_size=500))
    first.train(files, batch_bytes=10_000)
    first.save_lossless(tmp_path / "v1")
    model = BBPEModel.from_file_lossless(tmp_path / "v1")
    plain = BBPETrainer(config()).train_from(model, files)
    got = BBPETrainer(config()).train_from(model, files, batch_bytes=4096)
    assert got.merges == plain.merges and got.vocab == plain.vocab
    assert got.merges[:len(model.merges)] == model.merges and len(got.merges) == 743
    one = dict(chunk_size_bytes=1 << 30)  # one chunk: the reference-made golden merges
    first = BBPETrainer(config(vocab_size=500, **one))
    first.train(files, batch_bytes=1 << 30)
    first.save_lossless(tmp_path / "v1one")
    assert BBPETrainer(config(**one)).train_from(BBPEModel.from_file_lossless(tmp_path / "v1one"), files, batch_bytes=1 << 20).merges == g1
    # a new corpus: the naive continuation (literal replay of the model's merges, then a plain BPE loop)
    new = [golden_dir / "data/sample.txt", golden_dir / "data/unicode.txt"]
    t = BBPETrainer(config(vocab_size=560, chunk_size_bytes=64))
    got = t.train_from(model, new, batch_bytes=128)
    new_words = [bytes(s) for s in t._preprocess_corpus(new)]
    exp_vocab, exp_merges = rh.resume_naive(new_words, helpers.base_tokens(SP), model.merges, 560 - 257 - len(model.merges), 1)
    assert got.merges == exp_merges and got.vocab == exp_vocab
    (tmp_path / "empty.txt").write_bytes(b"")
    same = BBPETrainer(config()).train_from(model, [tmp_path / "empty.txt"], batch_bytes=4096)
    assert same.merges == model.merges and same.vocab == model.vocab
