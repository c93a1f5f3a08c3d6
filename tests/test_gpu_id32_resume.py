"""GPU (-m gpu): the u32 resumed load (id_bits = 32 with yabpe_load_words_resumed: id32_load with merges, rp32_lookup, the
one-lane-per-word replay of k32_words, k32_word_slots, k32_build_tiles, k32_place_words) through the C ABI at
small sizes, with merges that DO match inside the words.  Every expected value is computed on the CPU (golden vectors, the C
oracle, the literal replay and naive continuation of tests/resume_helpers.py, tests/limit_helpers.py, tie_helpers.replay),
never by the u16 path; every comparison is exact: merges, vocabulary and ids.  Every context runs with verify = 1 and checks
yabpe_verify_table after the load and after the training.  tests/test_id32_handover_inputs.py pins, on the CPU, what the
inputs below are chosen for."""
from __future__ import annotations

import numpy as np
import pytest

from tests import handover_helpers as hh
from tests import helpers, id32_helpers, limit_helpers as lh, resume_helpers as rh

pytestmark = pytest.mark.gpu
SP = hh.SP
ID32 = id32_helpers.ID32
E_INVALID = -1


def resumed32(words, freq, base, merges, budget, min_frequency, dedup=False, options=None):
    return rh.resumed_train(words, freq, base, merges, budget, min_frequency, dedup=dedup, options={**ID32, **(options or {})})


def id_order(base, merges) -> dict:
    from yet_another_bpe import _native

    return {t: i for i, t in enumerate(_native.merge_triples(base, merges)[0])}


# ---------------------------------------------------------------- 1. corpus.en from several split points
@pytest.fixture(scope="module")
def corpus_en(golden_dir):
    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")
    words, freq = helpers.pooled(helpers.corpus_en_words())
    base = helpers.base_tokens(SP)
    return g1, words, freq, base, id_order(base, g1)


@pytest.mark.parametrize("v1", [1, 100, 4439, 8000])
def test_corpus_en_to_exhaustion_from_several_split_points(corpus_en, v1):
    g1, words, freq, base, want_vocab = corpus_en
    vocab, merges, rs, st = resumed32(words, freq, base, g1[:v1], 10 ** 5, 1)
    assert merges == g1
    assert vocab == want_vocab
    assert rs["tokens"] == sum(len(rh.literal_replay(w, g1[:v1])) for w in words)
    assert rs["n_unique"] == len(words)
    assert st["n_tiles"] >= 3  # (k32_build_tiles across SPAN32 boundaries)


# ---------------------------------------------------------------- 2. small tie-heavy corpora with specials
def test_random_small_resumed_vs_oracle():
    """40 corpora of the recipe of test_random_small_vs_oracle (handover_helpers.random_small): resumed from the oracle's
    first k merges for k = 1, half and all but one, with the rest of the budget, the result is the oracle's whole model."""
    ran = 0
    for t, (words, sp, vs, mf, exp_vocab, exp_merges) in enumerate(hh.random_small()):
        if len(exp_merges) < 3:
            continue
        ran += 1
        base = helpers.base_tokens(sp)
        uw, fq = helpers.pooled(words)
        for k in (1, len(exp_merges) // 2, len(exp_merges) - 1):
            vocab, merges, rs, _st = resumed32(uw, fq, base, exp_merges[:k], vs - len(base) - k, mf)
            assert merges == exp_merges and vocab == exp_vocab, (t, k)
            assert rs["tokens"] == sum(len(rh.literal_replay(w, exp_merges[:k])) for w in uw), (t, k)
    assert ran >= 30


# ---------------------------------------------------------------- 3. reused ids on both sides of the split
@pytest.mark.parametrize("name", ["ab_ab", "abc_abc_bc", "abc_many", "abcdef_pairs"])
def test_reused_ids_on_both_sides_of_the_split(name):
    """Resumed directly before and directly after every merge that reused an id, and once past the last: the replayed triples
    then hold merges whose result id is smaller than an operand's, and the u32 selection reuses the later ones itself."""
    c = hh.reuse_case(name)
    freq = np.array(c["freqs"], dtype=np.uint64)
    for k in hh.reuse_splits(c):
        vocab, merges, rs, _st = resumed32(c["types"], freq, c["base"], c["merges"][:k], c["budget"] - k, 1)
        assert merges == c["merges"] and vocab == c["vocab"], (name, k)
        assert rs["tokens"] == sum(len(rh.literal_replay(w, c["merges"][:k])) for w in c["types"]), (name, k)


def test_a_merge_whose_operand_appears_only_later_is_not_applied():
    """handover_helpers.late_operand_case: the model's first merge (abc, d) names the special "abc", which the words hold only
    after the model's last merge (ab, c) reused its id.  The literal replay leaves "abc d" (the rank of (abc, d) has passed:
    the rank floor of rp32_lookup); the continuation then learns (abc, d) itself, a second rank of the same pair, and is
    resumed once more behind it."""
    c = hh.late_operand_case()
    freq = np.array(c["freqs"], dtype=np.uint64)
    for k in (3, 4, 6):
        model = c["all_merges"][:k]
        vocab, merges, rs, _st = resumed32(c["words"], freq, c["base"], model, c["budget"] - (k - 3), 1)
        assert rs["tokens"] == sum(len(rh.literal_replay(w, model)) for w in c["words"]), k
        assert merges == c["all_merges"] and vocab == c["vocab"], k


# ---------------------------------------------------------------- 4. the long-word boundary after a replay
@pytest.mark.parametrize("form", ["host_pooled", "device_dedup"])
@pytest.mark.parametrize("k", hh.LONG_SPLITS)
def test_long_word_boundary_after_a_replay(k, form):
    """Words of exactly 63 and 64 tokens after the replay (k = 5, 12), words that are long by bytes and short by tokens:
    n_long counts tokens after the replay, and the model is the oracle's."""
    words = list(hh.long_words())
    _ref_vocab, ref = hh.long_reference()
    base = helpers.base_tokens(SP)
    if form == "host_pooled":
        uw, fq = helpers.pooled(words)
        vocab, merges, rs, _st = resumed32(uw, fq, base, ref[:k], 150, 1)
    else:
        vocab, merges, rs, _st = resumed32(words, None, base, ref[:k], 150, 1, dedup=True)
    lengths = hh.long_lengths(k)
    assert rs["n_unique"] == len(lengths) and rs["tokens"] == sum(lengths.values())
    assert rs["n_long"] == sum(1 for n in lengths.values() if n >= hh.LONG)
    assert merges == ref[:k + 150]
    assert vocab == id_order(base, ref[:k + 150])


# ---------------------------------------------------------------- 5. a new corpus
def test_new_corpus_equals_the_naive_continuation():
    from yet_another_bpe import _native

    words_a, words_b, (vocab_a, merges_a), (want_vocab, want_merges) = hh.new_corpus()
    _spec_a, spec_b, n_a, n_b = hh.new_corpus_specs()
    base = helpers.base_tokens(SP)
    assert len(merges_a) == n_a and len(want_merges) - n_a >= n_b - 15
    uw, fq = helpers.pooled(words_b)
    vocab, merges, _rs, _st = resumed32(uw, fq, base, merges_a, n_b, 2)
    assert merges == want_merges and vocab == want_vocab
    assert all(vocab[t] == i for t, i in vocab_a.items())  # old ids unchanged
    # pooled on the device
    vocab_d, merges_d, _rs, _st = resumed32(words_b, None, base, merges_a, n_b, 2, dedup=True)
    assert merges_d == want_merges and vocab_d == want_vocab
    # the words as device pointers that another context owns
    toks, triples = _native.merge_triples(base, merges_a)
    with _native.Context() as gen:
        db, do, nw, nb = gen.synth_generate(spec_b.target_bytes, spec_b.n_types, spec_b.seed, spec_b.alphabet, spec_b.space_prefix)
        assert nw == len(words_b) and gen.d2h(db, nb).tobytes() == b"".join(words_b)
        with _native.Context() as ctx:
            for name, value in ID32.items():
                ctx.set_option(name, value)
            ctx.set_vocab(toks)
            ctx.load_words_resumed_ptr(db, do, nw, triples, dedup=True)
            assert ctx.verify_table() == 0
            assert ctx.resume_stats()["n_unique"] == len(uw)
            left, right, merged, _count = ctx.train(n_b, 2)
            assert ctx.verify_table() == 0
    vocab_p, new = _native.decode_merges(toks, left, right, merged)
    assert list(merges_a) + new == want_merges and vocab_p == want_vocab


# ---------------------------------------------------------------- 6. degenerate inputs
def test_words_that_are_one_token_after_the_replay():
    base = helpers.base_tokens(SP)
    merges = [(b"a", b"b"), (b"ab", b"c")]
    # a corpus of only such words: no pairs, zero new merges, a clean return
    vocab, out, rs, st = resumed32([b"abc", b"ab", b"a", b"c"], np.array([5, 4, 3, 2], dtype=np.uint64), base, merges, 50, 1)
    assert out == merges and rs["tokens"] == 4 and st["table_entries"] == 0
    assert vocab == id_order(base, merges)
    # ... and mixed with words that still hold pairs
    words = [b"abc", b"abcabc", b"ab", b"xabcx", b"x"]
    freq = np.array([5, 4, 3, 2, 9], dtype=np.uint64)
    vocab, out, rs, _st = resumed32(words, freq, base, merges, 50, 1)
    want_vocab, want = rh.naive_continue({rh.literal_replay(w, merges): int(f) for w, f in zip(words, freq)}, id_order(base, merges), 50, 1)
    assert out == merges + want and vocab == want_vocab and rs["tokens"] == 1 + 2 + 1 + 3 + 1


def test_no_merges_behaves_as_load_words(corpus_en):
    from yet_another_bpe import _native

    g1, words, freq, base, _v = corpus_en
    flat, off = helpers.flatten(words)
    empty = tuple(np.zeros(0, dtype=np.uint32) for _ in range(3))
    out = []
    for resumed in (False, True):
        with _native.Context() as ctx:
            for name, value in ID32.items():
                ctx.set_option(name, value)
            ctx.set_vocab(base)
            if resumed:
                ctx.load_words_resumed(flat, off, freq, empty)
            else:
                ctx.load_words(flat, off, freq)
            assert ctx.verify_table() == 0
            left, right, merged, count = ctx.train(300, 1)
            out.append((left.tolist(), right.tolist(), merged.tolist(), count.tolist()))
    assert out[0] == out[1]
    assert _native.decode_merges(base, *(np.array(x, dtype=np.uint32) for x in out[1][:3]))[1] == g1[:300]


def test_refused_calls():
    from yet_another_bpe import _native

    base = helpers.base_tokens(SP)
    toks, triples = _native.merge_triples(base, [(b"a", b"b"), (b"ab", b"c")])
    flat, off = helpers.flatten([b"abc", b"abcabc", b"cab"])
    freq = np.array([3, 2, 1], dtype=np.uint64)
    with _native.Context() as ctx:
        for name, value in ID32.items():
            ctx.set_option(name, value)
        ctx.set_vocab(toks)
        bad = tuple(x.copy() for x in triples)
        bad[2][1] = len(toks)  # an id the vocabulary does not have
        with pytest.raises(_native.YabpeError) as e:
            ctx.load_words_resumed(flat, off, freq, bad)
        assert e.value.code == E_INVALID
        bad = tuple(x.copy() for x in triples)
        bad[2][1] = toks.index(b"ab")  # (ab, c) -> a token of two bytes
        with pytest.raises(_native.YabpeError) as e:
            ctx.load_words_resumed(flat, off, freq, bad)
        assert e.value.code == E_INVALID and "bytes" in str(e.value)
        ctx.load_words_resumed(flat, off, freq, triples)  # the context is still usable
        assert ctx.verify_table() == 0
        assert ctx.resume_stats()["tokens"] == 1 + 2 + 2
        left, right, merged, _count = ctx.train(10, 1)
    # abc x3, abc abc x2, c ab x1: (abc, abc) 2, (c, ab) 1
    assert _native.decode_merges(toks, left, right, merged)[1] == [(b"abc", b"abc"), (b"c", b"ab")]


# ---------------------------------------------------------------- 7. a maximum token length with a resumed load
@pytest.mark.parametrize("limit", [4, 16])
def test_max_token_bytes_after_a_replay(limit):
    """The model's merges (up to 11 bytes) are replayed whatever their length; only the merges learned now obey the limit."""
    uw, fq, model = hh.limit_model()
    want_vocab, want_merges = hh.limit_continuation(limit)
    vocab, merges, _rs, _st = resumed32(uw, fq, helpers.base_tokens(lh.SP), model, hh.LIMIT_MORE, 1, options={"max_token_bytes": limit})
    assert merges == want_merges and vocab == want_vocab
