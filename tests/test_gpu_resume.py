"""GPU: continuing from a trained model (yabpe_load_words_resumed / BBPETrainer.train_from).  Training to V2 from scratch
must equal training to V1 < V2, saving losslessly, loading and continuing to V2 -- merge for merge, id for id -- on the G1
corpus, on lexicon text through files, and on the quarter-GiB G10 twin (its pins); on a NEW corpus the result must equal the
naive continuation of tests/resume_helpers.py (literal replay of the model's merges, then a plain BPE loop)."""
from __future__ import annotations

import hashlib
import json
from collections import Counter

import numpy as np
import pytest

from oracle import oracle
from tests import helpers, resume_helpers as rh

pytestmark = pytest.mark.gpu

SP = ["<|endoftext|>"]
E_INVALID, E_CAPACITY = -1, -4


resumed_train = rh.resumed_train  # (shared with tests/test_gpu_id32_resume.py, which sets id_bits = 32)


@pytest.mark.parametrize("v1", [1, 100, 743, 4439, 8000])
def test_corpus_en_to_exhaustion_from_several_split_points(golden_dir, v1):
    from yet_another_bpe import _native

    g1 = helpers.read_hex_merges(golden_dir / "g1_corpus_en_exhaustive.hex")
    meta = json.loads((golden_dir / "g1_meta.json").read_text())
    words, freq = helpers.pooled(helpers.corpus_en_words())
    base = helpers.base_tokens(SP)
    vocab, merges, rs, _st = resumed_train(words, freq, base, g1[:v1], 10 ** 5, 1)
    assert merges == g1
    for k, sha in meta["sha256"].items():
        assert hashlib.sha256(oracle.merges_hex(merges[: int(k)]).encode()).hexdigest() == sha
    assert vocab == {t: i for i, t in enumerate(_native.merge_triples(base, g1)[0])}
    assert rs["n_unique"] == len(words) and rs["tokens"] == sum(len(rh.literal_replay(w, g1[:v1])) for w in words)


def test_lexicon_text_through_files_train_from_equals_train(tmp_path, monkeypatch):
    from yet_another_bpe import _native, synth
    from yet_another_bpe.trainer import BBPEModel, BBPETrainer, BBPETrainerConfig

    monkeypatch.setenv("YABPE_PRETOKENIZE", "gpu")
    lb, lo = synth.text_lexicon(30000, 11)
    with _native.Context() as gen:
        tb, _to, _np, tn = gen.synth_generate_lex(16 << 20, 11, lb, lo)
        gen.d2h(tb, tn).tofile(tmp_path / "text.txt")
    cfg = dict(min_frequency=2, max_workers=2, chunk_size_bytes=4 << 20, special_tokens=SP)
    v1, v2 = 257 + 1500, 257 + 4000
    full = BBPETrainer(BBPETrainerConfig(vocab_size=v2, **cfg)).train([tmp_path / "text.txt"])
    assert len(full.merges) == 4000
    first = BBPETrainer(BBPETrainerConfig(vocab_size=v1, **cfg))
    part = first.train([tmp_path / "text.txt"])
    assert part.merges == full.merges[:1500]
    first.save_lossless(tmp_path / "v1")
    second = BBPETrainer(BBPETrainerConfig(vocab_size=v2, **cfg))
    out = second.train_from(BBPEModel.from_file_lossless(tmp_path / "v1"), [tmp_path / "text.txt"])
    assert out.merges == full.merges and out.vocab == full.vocab and out.special_tokens == SP
    second.save_lossless(tmp_path / "v2")
    again = BBPEModel.from_file_lossless(tmp_path / "v2")
    assert again.merges == full.merges and again.vocab == full.vocab
    # a zero budget and an empty corpus return the model unchanged
    (tmp_path / "empty.txt").write_bytes(b"")
    same = BBPETrainer(BBPETrainerConfig(vocab_size=v2 + 10, **cfg)).train_from(again, [tmp_path / "empty.txt"])
    assert same.merges == full.merges and same.vocab == full.vocab


def test_g10_quarter_gib_resumed_at_10000(golden_dir):
    """The quarter-GiB G10 twin: 10,000 merges, the context torn down, a fresh one resumed to 50,000 -- against the pins of
    the from-scratch job (its 268 k-class long words take the sequential walk and, where they still hold 64 tokens or
    more after the replay, the token-count long path)."""
    from yet_another_bpe import _native, synth
    from yet_another_bpe.trainer import BBPETrainer, chunk_ranges

    meta = json.loads((golden_dir / "g10_config5_0.25gib_meta.json").read_text())
    g, sp = meta["generator"], meta["special_tokens"]
    base = helpers.base_tokens(sp)
    lb, lo = synth.text_lexicon(g["n_types"], g["seed"])
    split = 10000
    with _native.Context() as gen:
        tb, _to, _n_pieces, tn = gen.synth_generate_lex(g["target_bytes"], g["seed"], lb, lo)
        assert tn == meta["text_bytes"]
        ranges = chunk_ranges(tn, meta["chunk_size_bytes"], lambda off, n: gen.d2h(tb + off, n).tobytes())
        dt, do, nw = gen.pretokenize(tb, n_bytes=tn, chunk_starts=[a for a, _ in ranges], special_tokens=sp)
        assert nw == meta["pretokens"]
        with _native.Context() as ctx:
            ctx.set_vocab(base)
            ctx.load_words_ptr(dt, do, nw, dedup=True)
            l0, r0, m0, _c0 = ctx.train(split, meta["min_frequency"])
            assert len(l0) == split
            trained = ctx.stream_checksum()
            tokens_trained = ctx.stats()["tokens_now"]
        toks, first = BBPETrainer._decode_merges(base, l0, r0, m0)
        toks = sorted(toks, key=toks.get)
        toks2, triples = _native.merge_triples(base, first)
        assert toks2 == toks and np.array_equal(triples[0], l0) and np.array_equal(triples[1], r0) and np.array_equal(triples[2], m0)
        with _native.Context() as ctx:
            ctx.set_vocab(toks)
            ctx.load_words_resumed_ptr(dt, do, nw, triples, dedup=True)
            rs = ctx.resume_stats()
            assert ctx.verify_table() == 0
            assert ctx.stream_checksum() == trained
            assert rs["n_unique"] == meta["unique_words"] and rs["tokens"] == tokens_trained and 0 < rs["n_long"] <= meta["unique_long_words"]
            l1, r1, m1, c1 = ctx.train(meta["n_merges"] - split, meta["min_frequency"])
            assert ctx.verify_table() == 0
        print(f"resumed load at {split} merges: segment {rs['segment_ms']:.1f} ms, build {rs['build_ms']:.1f} ms, long words {rs['n_long']}")
    left, right, merged = np.concatenate([l0, l1]), np.concatenate([r0, r1]), np.concatenate([m0, m1])
    assert len(left) == meta["n_merges"] and int(c1[-1]) == meta["last_count"]
    assert hashlib.sha256(left.astype(np.uint32).tobytes() + right.astype(np.uint32).tobytes() + merged.astype(np.uint32).tobytes()).hexdigest() == meta["id_triples_sha256"]
    vocab, merges = BBPETrainer._decode_merges(base, left, right, merged)
    lines = oracle.merges_hex(merges).splitlines(keepends=True)
    for k in ("32000", "50000"):
        assert hashlib.sha256("".join(lines[: int(k)]).encode()).hexdigest() == meta["merges_sha256"][k], f"first {k} merges differ from the oracle"
    assert len(vocab) == meta["vocab_size"]


def test_new_corpus_equals_the_naive_continuation():
    from yet_another_bpe import _native, synth
    from yet_another_bpe.tokenizer import BBPETokenizer

    def words_of(spec):
        flat, off = synth.generate(spec)
        fb, o = flat.tobytes(), off.tolist()
        return [fb[o[i]:o[i + 1]] for i in range(len(o) - 1)]

    words_a = words_of(synth.SynthSpec(300 << 10, 4000, 5, b"abcdefghijklmnopqrstuvwxyz", True))
    words_b = words_of(synth.SynthSpec(300 << 10, 3000, 77, b"aeioubcdxyz0123456789-", True))
    base = helpers.base_tokens(SP)
    fa, oa = helpers.flatten(words_a)
    vocab_a, merges_a = _native.train_words(fa, oa, None, base, 600, 2, dedup=True)
    assert len(merges_a) == 600
    pooled_b, freq_b = helpers.pooled(words_b)
    vocab, merges, _rs, _st = resumed_train(pooled_b, freq_b, base, merges_a, 350, 2)
    want_vocab, want_merges = rh.resume_naive(words_b, base, merges_a, 350, 2)
    assert len(merges) - len(merges_a) >= 300
    assert merges == want_merges and vocab == want_vocab
    assert all(vocab[t] == i for t, i in vocab_a.items())  # old ids unchanged
    # pooling on the device gives the same
    fb, ob = helpers.flatten(words_b)
    vocab_d, merges_d, _rs, _st = resumed_train(words_b, None, base, merges_a, 350, 2, dedup=True)
    assert merges_d == merges and vocab_d == vocab
    tok = BBPETokenizer(vocab=vocab, merges=merges, special_tokens=SP)
    docs = [b"".join(words_b[a:a + 500]).decode() for a in range(0, 5000, 500)]
    ids = tok.encode_batch_device(docs)
    assert ids == tok.encode_batch(docs)
    assert tok.decode_batch_device(ids) == docs


def test_no_merges_behaves_as_load_words(golden_dir):
    from yet_another_bpe import _native

    words, freq = helpers.pooled(helpers.corpus_en_words())
    base = helpers.base_tokens(SP)
    flat, off = helpers.flatten(words)
    empty = tuple(np.zeros(0, dtype=np.uint32) for _ in range(3))
    out = []
    for resumed in (False, True):
        with _native.Context() as ctx:
            ctx.set_vocab(base)
            if resumed:
                ctx.load_words_resumed(flat, off, freq, empty)
            else:
                ctx.load_words(flat, off, freq)
            chk = ctx.stream_checksum()
            left, right, merged, count = ctx.train(300, 1)
            out.append((chk, left.tolist(), right.tolist(), merged.tolist(), count.tolist()))
    assert out[0] == out[1]


def test_refused_calls():
    from yet_another_bpe import _native

    base = helpers.base_tokens(SP)
    toks, triples = _native.merge_triples(base, [(b"a", b"b"), (b"ab", b"c")])
    words = [b"abc", b"abcabc", b"cab"]
    flat, off = helpers.flatten(words)
    freq = np.array([3, 2, 1], dtype=np.uint64)
    with _native.Context() as ctx:
        ctx.set_vocab(toks)
        with pytest.raises(_native.YabpeError) as e:  # the flat layout
            ctx.load_words_resumed(flat, off, None, triples)
        assert e.value.code == E_INVALID and "pooled" in str(e.value)
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


def test_id_space_exhausted_is_reported_not_truncated():
    from yet_another_bpe import _native

    base = helpers.base_tokens([])
    letters = set(b"abc")
    pairs = [(bytes([x]), bytes([y])) for x in range(256) if x not in letters for y in range(256)]
    pairs += [(bytes([x]), bytes([y])) for x in letters for y in range(256) if y not in letters]
    merges = pairs[:65270]
    toks, triples = _native.merge_triples(base, merges)
    assert len(toks) == 256 + 65270 == 65534 - 8  # the id space holds 65,534 tokens (ids 0 .. 65,533): 8 ids are left
    import random
    rng = random.Random(3)
    words = [bytes(rng.choice(b"abc") for _ in range(rng.randint(2, 12))) for _ in range(400)]
    words, freq = helpers.pooled(words)
    flat, off = helpers.flatten(words)
    with _native.Context() as ctx:
        ctx.set_vocab(toks)
        ctx.load_words_resumed(flat, off, freq, triples)
        assert ctx.verify_table() == 0
        with pytest.raises(_native.YabpeError) as e:
            ctx.train(100, 1)
        assert e.value.code == E_CAPACITY and "id space" in str(e.value)
        # nothing was truncated or wrapped: the 8 ids that were left are taken, every one names a token of the corpus'
        # letters, and the model's tokens are as they were
        n = ctx.n_tokens()
        print("tokens after the refused job:", n)
        assert n == 65534
        assert [ctx.token_bytes(i) for i in (256, 30000, len(toks) - 1)] == [toks[256], toks[30000], toks[-1]]
        for i in range(len(toks), n):
            t = ctx.token_bytes(i)
            assert len(t) >= 2 and set(t) <= set(b"abc")


def test_words_that_are_one_token_after_the_replay():
    from yet_another_bpe import _native

    base = helpers.base_tokens(SP)
    merges = [(b"a", b"b"), (b"ab", b"c")]
    # a corpus of only such words: no pairs, zero new merges, a clean return
    vocab, out, rs, st = resumed_train([b"abc", b"ab", b"a", b"c"], np.array([5, 4, 3, 2], dtype=np.uint64), base, merges, 50, 1)
    assert out == merges and rs["tokens"] == 4 and st["table_entries"] == 0
    assert vocab == {t: i for i, t in enumerate(_native.merge_triples(base, merges)[0])}
    # ... and mixed with words that still hold pairs
    words = [b"abc", b"abcabc", b"ab", b"xabcx", b"x"]
    freq = np.array([5, 4, 3, 2, 9], dtype=np.uint64)
    vocab, out, rs, _st = resumed_train(words, freq, base, merges, 50, 1)
    want_vocab, want = rh.naive_continue({rh.literal_replay(w, merges): int(f) for w, f in zip(words, freq)},
                                         {t: i for i, t in enumerate(_native.merge_triples(base, merges)[0])}, 50, 1)
    assert out == merges + want and vocab == want_vocab and rs["tokens"] == 1 + 2 + 1 + 3 + 1
