"""GPU (-m gpu): the u32-id merge loop (option id_bits = 32) through the C ABI, bit-exact against the golden
vectors, the C oracle and the plain-Python references of the helper modules: merges AND id assignment, no tolerance.  Every
context runs with verify = 1 (the incremental pair table equals a recount after every yabpe_train)."""
from __future__ import annotations

import random

import numpy as np
import pytest

from oracle import oracle
from tests import big_count_helpers as bc
from tests import helpers, id32_helpers, limit_helpers as lh, resume_helpers, tie_helpers

pytestmark = pytest.mark.gpu
SP = ["<|endoftext|>"]
ID32 = id32_helpers.ID32
E_INVALID, E_CAPACITY = -1, -4
WORD_LIMIT = 63  # tokens of the longest word the tile stream keeps (csrc/yabpe_id32_kernels.h: LMAX32 - 1)


def gpu_train(words, freq, vocab_size, min_frequency, specials, dedup=False, options=None, want_stats=False):
    from yet_another_bpe import _native

    base = helpers.base_tokens(specials)
    flat, off = helpers.flatten(words)
    return _native.train_words(flat, off, freq, base, max(0, vocab_size - len(base)), min_frequency, dedup=dedup,
                               options={**ID32, **(options or {})}, want_stats=want_stats)


# ---------------------------------------------------------------- 1. golden cases, three input forms
@pytest.mark.parametrize("form", ["no_counts", "host_pooled", "device_dedup"])
def test_golden_cases(form):
    for c in helpers.golden_cases():
        if not c["words_b"]:
            continue
        if form == "host_pooled":
            uw, fq = helpers.pooled(c["words_b"])
            vocab, merges = gpu_train(uw, fq, c["vocab_size"], c["min_frequency"], c["special_tokens"])
        else:
            vocab, merges = gpu_train(c["words_b"], None, c["vocab_size"], c["min_frequency"], c["special_tokens"], dedup=(form == "device_dedup"))
        assert merges == c["merges_b"], (form, c["name"])
        assert len(vocab) == c["vocab_len"], (form, c["name"])
        assert {k: v for k, v in vocab.items() if v >= 256} == c["vocab_b"], (form, c["name"])


# ---------------------------------------------------------------- 2. random small alphabets, tie-heavy corpora
def test_random_small_vs_oracle():
    """The recipe of tests/test_gpu_parity.py::test_random_small_vs_oracle with another seed: 120 corpora over small alphabets
    (0x00 / 0xFF included), 1 .. 40 word types of 1 .. 30 bytes repeated 1 .. 6 times, specials that are or become tokens."""
    rng = random.Random(3211)
    for t in range(120):
        al = rng.choice([b"ab", b"abc", b"xyz ", bytes([0, 255, 254, 1]), b"abcdefghijklmnop"])
        words = []
        for _ in range(rng.randint(1, 40)):
            words += [bytes(rng.choice(al) for _ in range(rng.randint(1, 30)))] * rng.randint(1, 6)
        rng.shuffle(words)
        sp = rng.choice([[], ["ab"], ["<|x|>"], ["a", "b"], ["[PAD]", "[UNK]", "[BOS]", "[EOS]"]])
        vs, mf = 256 + rng.randint(0, 120), rng.randint(1, 3)
        exp = oracle.merge_loop(words, vs, mf, sp)
        assert gpu_train(words, None, vs, mf, sp) == exp, t
        uw, fq = helpers.pooled(words)
        assert gpu_train(uw, fq, vs, mf, sp) == exp, t


@pytest.mark.parametrize("name", ["stems", "plateau", "levels"])
def test_tie_heavy_corpora(name):
    words = getattr(tie_helpers, name)()
    exp = oracle.merge_loop(words, 256 + 400, 1, [])
    assert gpu_train(words, None, 256 + 400, 1, [], dedup=True) == exp
    types, freqs = getattr(tie_helpers, name + "_types")()
    assert gpu_train(list(types), np.array(freqs, dtype=np.uint64), 256 + 400, 1, []) == exp


def test_tie_heavy_reused_ids():
    for name, types, freqs, specials in tie_helpers.reuse_cases():
        words = [w for w, f in zip(types, freqs) for _ in range(f)]
        exp = oracle.merge_loop(words, 256 + len(specials) + 200, 1, list(specials))
        assert gpu_train(list(types), np.array(freqs, dtype=np.uint64), 256 + len(specials) + 200, 1, list(specials)) == exp, name


# ---------------------------------------------------------------- 3. corpus.en to exhaustion
# the selection's two forms: the whole table per merge (what a table below "cand_min_slots" gets), and the candidate list --
# with room for everything, and with 16 entries, so that it overflows, drains and is rebuilt all the time
CAND = {"table": {}, "list": {"cand_min_slots": 0}, "list16": {"cand_min_slots": 0, "cand_cap": 16, "check_interval": 3}}


@pytest.mark.parametrize("form", list(CAND))
def test_corpus_en_exhaustive(golden_dir, form):
    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")
    words = helpers.corpus_en_words()
    vocab, merges, st = gpu_train(words, None, 257 + 9000, 1, SP, dedup=True, options=CAND[form], want_stats=True)
    assert len(merges) == 8199 and merges == g1
    assert (st["cand_rebuilds"] > 0) == (form != "table"), st["cand_rebuilds"]
    _, m2 = gpu_train(words, None, 257 + 9000, 2, SP, dedup=True, options=CAND[form])
    assert m2 == g1[:4439]


@pytest.mark.parametrize("form", ["list", "list16"])
def test_candidate_list_on_small_and_tie_heavy_corpora(form):
    for c in helpers.golden_cases()[::7]:
        if c["words_b"]:
            vocab, merges = gpu_train(c["words_b"], None, c["vocab_size"], c["min_frequency"], c["special_tokens"], options=CAND[form])
            assert merges == c["merges_b"] and {k: v for k, v in vocab.items() if v >= 256} == c["vocab_b"], (form, c["name"])
    for name in ("stems", "plateau", "levels"):
        types, freqs = getattr(tie_helpers, name + "_types")()
        words = [w for w, f in zip(types, freqs) for _ in range(f)]
        assert gpu_train(list(types), np.array(freqs, dtype=np.uint64), 256 + 400, 1, [], options=CAND[form]) == oracle.merge_loop(words, 256 + 400, 1, []), (form, name)
    for name, types, freqs, specials in tie_helpers.reuse_cases():
        words = [w for w, f in zip(types, freqs) for _ in range(f)]
        exp = oracle.merge_loop(words, 256 + len(specials) + 200, 1, list(specials))
        assert gpu_train(list(types), np.array(freqs, dtype=np.uint64), 256 + len(specials) + 200, 1, list(specials), options=CAND[form]) == exp, (form, name)


# ---------------------------------------------------------------- 4. long words
def test_long_words():
    rng = random.Random(77)
    words = [bytes(rng.choice(b"abcdefgh") for _ in range(n)) for n in (64, 65, 100, 129, 200, 257, 300)]
    words += [b"z" * 500, b"q" * (WORD_LIMIT - 1), b"q" * WORD_LIMIT, b"q" * (WORD_LIMIT + 1), b"ab" * 31 + b"a", b"ab" * 32]
    words += [b"abcabc"] * 7 + [b"aaa", b"zz"]
    exp = oracle.merge_loop(words, 257 + 150, 1, SP)
    vocab, merges, st = gpu_train(words, None, 257 + 150, 1, SP, want_stats=True)
    assert (vocab, merges) == exp
    assert st["n_long_words"] == sum(1 for w in words if len(w) > WORD_LIMIT)  # (no pooling asked: every occurrence is a word)
    uw, fq = helpers.pooled(words * 3)
    assert gpu_train(uw, fq, 257 + 150, 1, SP) == oracle.merge_loop(words * 3, 257 + 150, 1, SP)


# ---------------------------------------------------------------- 5. maximum token length
@pytest.mark.parametrize("limit", [2, 4, 16])
def test_max_token_bytes(limit):
    uw, fq = helpers.pooled(lh.en_words())
    exp_vocab, exp_merges = lh.train(uw, fq, 600, 1, SP, limit=limit)
    vocab, merges = gpu_train(uw, fq, 257 + 600, 1, SP, options={"max_token_bytes": limit})
    assert merges == exp_merges and vocab == exp_vocab


# ---------------------------------------------------------------- 6. growth paths
def test_growth_paths():
    from yet_another_bpe import synth

    flat, off = synth.generate(synth.SynthSpec(1 << 20, 8_000, 7, bytes(range(256)), False))
    base = helpers.base_tokens(SP)
    from yet_another_bpe import _native

    exp = oracle.train_flat(flat, off, 257 + 500, 1, SP)
    v, m, st = _native.train_words(flat, off, None, base, 500, 1, dedup=True, want_stats=True,
                                   options={**ID32, "table_min_log2": 10, "check_interval": 7, "retile_pct": 99, "retile_min_tiles": 4, "pool_bytes": 1024})
    assert (v, m) == exp
    # (pooled words over 256 letters lose about 2 % of their slots in 500 merges: the repack is asked for at 99 % fill)
    assert st["table_rebuilds"] >= 1 and st["retiles"] >= 1 and st["pool_growths"] >= 1, {k: st[k] for k in ("table_rebuilds", "retiles", "pool_growths", "n_tiles", "live_slots")}
    assert st["table_capacity"] > 1 << 10


# ---------------------------------------------------------------- 7. frequencies at 2^32 - 1, a pair count past 2^32
def test_big_counts():
    from yet_another_bpe import _native

    types, freqs = bc.named("small1")
    flat, off = helpers.flatten(list(types))
    exp_vocab, exp_merges, ids = bc.expected("small1", 400)
    with _native.Context() as ctx:
        for k, v in ID32.items():
            ctx.set_option(k, v)
        ctx.set_vocab(helpers.base_tokens(()))
        ctx.load_words(flat, off, bc.freq_array(freqs))
        left, right, merged, count = ctx.train(400, 1)
    assert max(freqs) == bc.F_MAX and int(count[0]) > 1 << 32
    for got, key in ((left, "left"), (right, "right"), (merged, "merged"), (count, "count")):
        assert np.array_equal(got, ids[key]), key


# ---------------------------------------------------------------- 8. crossing the u16 bound, resumed
def test_crossing_the_old_bound_resumed():
    from yet_another_bpe import _native

    base, model_merges, words, freq = id32_helpers.crossing_model()
    toks, triples = _native.merge_triples(base, model_merges)
    assert len(toks) == 65526
    flat, off = helpers.flatten(words)
    # resume_helpers.resume_naive(words, base, merges, 100, 1) without its 26 million no-op rewrites: no merge of the model can
    # match inside a word over abc (each names a byte outside), so the literal replay leaves the words as single bytes
    assert not any(set(l + r) <= set(b"abc") for l, r in model_merges)
    assert resume_helpers.literal_replay(words[0], model_merges[:300] + model_merges[-300:]) == tuple(bytes([x]) for x in words[0])
    seg = {tuple(bytes([x]) for x in w): int(f) for w, f in zip(words, freq)}
    exp_vocab, new_merges = resume_helpers.naive_continue(seg, {t: i for i, t in enumerate(toks)}, 100, 1)
    exp_merges = list(model_merges) + new_merges
    with _native.Context() as ctx:
        for k, v in ID32.items():
            ctx.set_option(k, v)
        ctx.set_vocab(toks)
        ctx.load_words_resumed(flat, off, freq, triples)
        assert ctx.verify_table() == 0
        left, right, merged, count = ctx.train(100, 1)
        n = ctx.n_tokens()
        new_tokens = [ctx.token_bytes(i) for i in range(len(toks), n)]
    vocab, merges = _native.decode_merges(toks, left, right, merged)
    assert list(model_merges) + merges == exp_merges
    assert vocab == exp_vocab and n == len(exp_vocab)
    fresh = [int(m) for m in merged if m >= len(toks)]
    assert fresh == list(range(65526, 65526 + len(fresh))) and fresh[-1] >= 65536  # 65,534, 65,535 and 65,536 without a gap
    assert all(exp_vocab[t] == len(toks) + i for i, t in enumerate(new_tokens))


# ---------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_context_usable():
    from yet_another_bpe import _native

    words = [b"abab", b"abc", b"bcbc"] * 5
    flat, off = helpers.flatten(words)
    exp = oracle.merge_loop(words, 256 + 20, 1, [])
    with _native.Context() as ctx:
        for k, v in ID32.items():
            ctx.set_option(k, v)
        ctx.set_vocab(helpers.base_tokens([]))
        with pytest.raises(_native.YabpeError) as e:
            ctx.set_option("id_bits", 16)
        assert e.value.code == E_INVALID
        ctx.set_option("id_bits", 32)  # (the value it has: accepted)
        ctx.load_words(flat, off)
        with pytest.raises(_native.YabpeError) as e:
            ctx.stream_dump()
        assert e.value.code == E_INVALID and "id_bits" in str(e.value)
        left, right, merged, _count = ctx.train(20, 1)
        assert _native.decode_merges(helpers.base_tokens([]), left, right, merged) == exp
    with _native.Context() as ctx:  # and the other way round
        ctx.set_vocab(helpers.base_tokens([]))
        with pytest.raises(_native.YabpeError) as e:
            ctx.set_option("id_bits", 32)
        assert e.value.code == E_INVALID
        ctx.load_words(flat, off)
        left, right, merged, _count = ctx.train(20, 1)
        assert _native.decode_merges(helpers.base_tokens([]), left, right, merged) == exp


def test_id_limit_is_reported():
    """Past the last id the result is YABPE_E_CAPACITY, as at 16 bits (the bound itself, 2^24 - 2 tokens, is lowered by the
    test option id32_limit: the same branch of the selection)."""
    from yet_another_bpe import _native

    flat, off = helpers.flatten([b"abcdefgh" * 4] * 3)
    with _native.Context() as ctx:
        for k, v in {**ID32, "id32_limit": 260}.items():
            ctx.set_option(k, v)
        ctx.set_vocab(helpers.base_tokens([]))
        ctx.load_words(flat, off)
        with pytest.raises(_native.YabpeError) as e:
            ctx.train(50, 1)
        assert e.value.code == E_CAPACITY and "id space" in str(e.value)
        assert ctx.n_tokens() == 260
