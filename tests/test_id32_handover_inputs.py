"""CPU: the conditions that tests/test_gpu_id32_resume.py and tests/test_gpu_id32_handover.py rely on, asserted from the
references alone (tests/handover_helpers.py): a changed recipe fails here, not on the GPU machine."""
from __future__ import annotations

import pytest

from tests import handover_helpers as hh
from tests import helpers, resume_helpers as rh

STAT_KEYS = ("id16_merges", "id16_stages", "id32_merges", "id32_replayed_merges")


def stages(*values) -> dict:
    return dict(zip(STAT_KEYS, values))


def test_stage_rule_on_scripted_lists():
    """expected_stages against the cases tests/test_id32_routes.py plays with its stub at full size"""
    assert hh.expected_stages(256, [True] * 65_278, 65_278, 65_534) is None
    assert hh.expected_stages(256, [True] * 66_304, 66_304, 65_534) == stages(65_278, 1, 1_026, 65_278)
    fresh = [k not in (10, 20, 65_279) for k in range(66_304)]
    assert hh.expected_stages(256, fresh, 66_304, 65_534) == stages(65_281, 3, 1_023, 65_281)
    assert hh.expected_stages(256, [True] * 300, 99_744, 65_534) == stages(300, 1, 0, 0)
    assert hh.expected_stages(256, [True] * (65_278 + 466), 466, 65_534, n_old=65_278) == stages(0, 0, 466, 65_278)
    assert hh.expected_stages(256, [True] * 44, 44, 65_534, mode="32") == stages(0, 0, 44, 0)


def test_random_small_corpora():
    cases = hh.random_small()
    assert len(cases) == 40 and sum(1 for c in cases if len(c[5]) >= 3) >= 30
    # specials that are tokens (no id) and specials that become tokens (a reused id in the replayed triples)
    assert any(len(helpers.base_tokens(c[1])) == 256 and c[1] for c in cases)
    assert any(not all(hh.fresh_flags(helpers.base_tokens(c[1]), c[5])) for c in cases)
    # ties: in most corpora some merge was chosen among equal counts by the byte order alone
    assert sum(1 for c in cases if len(set(c[0])) >= 2) >= 30


def test_reuse_cases_hits_and_stages():
    many, pairs = hh.reuse_case("abc_many"), hh.reuse_case("abcdef_pairs")
    assert (many["hits"], many["n_steps"]) == ([3, 4, 17, 20], 91)
    assert (pairs["hits"], pairs["n_steps"]) == ([0, 1, 3, 4, 11], 123)
    for name in ("ab_ab", "abc_abc_bc", "abc_many", "abcdef_pairs"):
        c = hh.reuse_case(name)
        assert c["hits"] and c["pairs"] == c["merges"] and len(c["merges"]) < c["budget"], name  # (replay and the oracle agree; exhaustion)
        assert [not f for f in hh.fresh_flags(c["base"], c["merges"])] == [k in c["hits"] for k in range(c["n_steps"])], name
        splits = hh.reuse_splits(c)
        assert all(h in splits and h + 1 in splits for h in c["hits"]) and splits[-1] > c["hits"][-1] + 1 and splits[-1] < len(c["merges"]), name
    assert not hh.reuse_case("ab_a_b")["hits"]
    # B2: h = 10 puts the first hits inside stage 1 (abcdef_pairs: the hit at merge 11 inside the first repeat), h = 2 at the seam
    want = {("abc_many", 10): stages(12, 2, 79, 12), ("abcdef_pairs", 10): stages(15, 3, 108, 15),
            ("abc_many", 2): stages(2, 1, 89, 2), ("abcdef_pairs", 2): stages(6, 4, 117, 6)}
    for (name, h), w in want.items():
        c = hh.reuse_case(name)
        fresh = [k not in c["hits"] for k in range(c["n_steps"])]
        assert hh.expected_stages(len(c["base"]), fresh, c["budget"], len(c["base"]) + h) == w, (name, h)
    # B7: the model's merges hold hits, the resumed stage 1 meets one more and repeats; or the bound lies below the model
    for name, (n_old, h), w, straight in (("abc_many", (8, 16), stages(11, 2, 72, 19), stages(0, 0, 83, 8)),
                                          ("abcdef_pairs", (6, 8), stages(7, 2, 110, 13), stages(0, 0, 117, 6))):
        c = hh.reuse_case(name)
        fresh = [k not in c["hits"] for k in range(c["n_steps"])]
        assert sum(1 for k in c["hits"] if k < n_old) >= 2
        assert hh.expected_stages(len(c["base"]), fresh, c["budget"] - n_old, len(c["base"]) + h, n_old=n_old) == w, name
        assert hh.expected_stages(len(c["base"]), fresh, c["budget"] - n_old, len(c["base"]) + 2, n_old=n_old) == straight, name


def test_inputs_that_tell_the_replay_rules():
    """The plain-Python per-word replay equals the literal replay on every input; without the leftmost rule it differs on
    words of the small corpora and of the reuse cases; without the rank floor only on the late-operand case (no corpus
    of these recipes ever needs it, which is why that case is written by hand)."""
    tell_leftmost = tell_floor = 0
    for words, _sp, _vs, _mf, _vocab, merges in hh.random_small():
        for k in (1, len(merges) // 2, len(merges) - 1) if len(merges) >= 3 else ():
            for w in set(words):
                lit = rh.literal_replay(w, merges[:k])
                assert hh.per_word_replay(w, merges[:k]) == lit
                tell_leftmost += hh.per_word_replay(w, merges[:k], leftmost=False) != lit
                tell_floor += hh.per_word_replay(w, merges[:k], rank_floor=False) != lit
    assert tell_leftmost >= 100 and tell_floor == 0
    for name in ("abc_many", "abcdef_pairs"):
        c = hh.reuse_case(name)
        assert any(hh.per_word_replay(w, c["merges"][:k], leftmost=False) != rh.literal_replay(w, c["merges"][:k])
                   for k in hh.reuse_splits(c) for w in c["types"]), name
    c = hh.late_operand_case()
    assert len(c["all_merges"]) > 6 and c["all_merges"][3] == c["merges"][0] == (b"abc", b"d")  # the same pair at two ranks
    for k in (3, 4, 6):
        model = c["all_merges"][:k]
        assert all(hh.per_word_replay(w, model) == rh.literal_replay(w, model) for w in c["words"])
    told = [w for w in c["words"] if hh.per_word_replay(w, c["merges"], rank_floor=False) != rh.literal_replay(w, c["merges"])]
    assert told == [b"abcd", b"abcdabcd", b"xabcd", b"abcabcd"] and rh.literal_replay(b"abcd", c["merges"]) == (b"abc", b"d")


def test_long_words_at_the_split_points():
    _vocab, ref = hh.long_reference()
    assert len(ref) == 300
    types = list(dict.fromkeys(hh.long_words()))
    assert sum(1 for w in types if len(w) > 63) == 10
    long_after = {k: sum(1 for n in hh.long_lengths(k).values() if n >= hh.LONG) for k in hh.LONG_SPLITS}
    assert long_after == {0: 10, 3: 9, 5: 7, 12: 6, 40: 5, 150: 3}
    for k in (5, 12):  # a word of exactly 63 tokens (the longest the tiles keep) and one of exactly 64 (the shortest long one)
        assert {63, 64} <= set(hh.long_lengths(k).values()), k
    assert sum(1 for n in hh.long_lengths(150).values() if n == 1) == 7
    # long by bytes, short by tokens: at every k > 0 some word over 63 bytes is tiled
    assert all(any(len(w) > 63 and n < hh.LONG for w, n in hh.long_lengths(k).items()) for k in hh.LONG_SPLITS[1:])


def test_new_corpus():
    words_a, words_b, (_vocab_a, merges_a), (_vocab, merges) = hh.new_corpus()
    assert len(merges_a) == 150 and len(merges) == 240
    # the model's merges do match inside the new words: the replay shortens them
    some = list(dict.fromkeys(words_b))[:200]
    assert sum(len(rh.literal_replay(w, merges_a)) for w in some) < sum(len(w) for w in some)


def test_limit_continuations():
    _uw, _fq, model = hh.limit_model()
    assert len(model) == hh.LIMIT_MODEL_MERGES and sum(1 for l, r in model if len(l + r) > 4) >= 10 and max(len(l + r) for l, r in model) < 16
    for limit in (4, 16):
        _vocab, merges = hh.limit_continuation(limit)
        assert merges[:len(model)] == model and len(merges) == len(model) + hh.LIMIT_MORE
        assert max(len(l + r) for l, r in merges[len(model):]) <= limit
    assert hh.limit_continuation(4)[1] != hh.limit_continuation(16)[1]
    vocab, merges = hh.limit4_reference()
    assert len(merges) == 300 and max(len(l + r) for l, r in merges) == 4


def test_tie_references_and_stop_points():
    for name, n in (("stems", 375), ("plateau", 400), ("levels", 400)):
        _types, _freqs, (_vocab, merges) = hh.tie_reference(name)
        assert len(merges) == n and all(hh.fresh_flags(helpers.base_tokens([]), merges)), name
    sp = hh.stop_points()
    counts = sp["counts"]
    assert all(a >= b for a, b in zip(counts, counts[1:]))
    min_frequency, j, h = sp["early"]
    assert j < h and counts[j - 1] >= min_frequency > counts[j]  # the job ends inside stage 1, after j merges
    min_frequency, j, h = sp["seam"]
    assert j == h + 1 and counts[j - 1] >= min_frequency > counts[j]  # ... after exactly one merge of stage 2
    assert sp["early"] == (3400, 3, 9) and sp["seam"] == (1640, 12, 11)


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    return hh.write_file(tmp_path_factory.mktemp("handover_inputs") / "corpus.txt")


@pytest.mark.parametrize("case", list(hh.FILE_CASES))
def test_file_pretokens_of_every_class(corpus_file, case):
    assert 32 << 10 <= corpus_file.stat().st_size <= 64 << 10  # several 4 KiB chunks per 8 KiB batch, several batches
    words = set(hh.file_words(corpus_file, **hh.FILE_CASES[case]))
    digits = [w.strip() for w in words if w.strip().isdigit()]
    assert digits and max(len(d) for d in digits) == 3  # 1234567 is cut into groups of three
    assert hh.SP[0].encode() in words
    if case == "o200k_base":  # the contraction stays with its word, words are cut where the case changes
        assert {b" don't", b" I'LL", b" foo", b"Bar", b" HTTPServer", b" cafe\xcc\x81"} <= words
    else:
        assert {b"'t", b"'ve", b" fooBar", b" HTTPServer"} <= words
        assert (b"'LL" in words) == (case != "gpt2_g3")  # contractions in either case: cl100k only
        if case == "cl100k_nfc":
            assert b" caf\xc3\xa9" in words and b" na\xc3\xafve" in words and not any(b"\xcc" in w for w in words)
        else:
            assert any(w.startswith(b"\xcc\x81") for w in words) and not any(b"\xc3" in w for w in words)
    vocab, merges = hh.file_reference(corpus_file, **hh.FILE_CASES[case])
    assert len(merges) == hh.FILE_MERGES == 200
    base = helpers.base_tokens(hh.SP)
    want = hh.expected_stages(len(base), hh.fresh_flags(base, merges), hh.FILE_MERGES, len(base) + hh.FILE_H)
    assert want["id16_merges"] >= hh.FILE_H and want["id32_merges"] == hh.FILE_MERGES - want["id16_merges"] > 100


def test_file_reference_of_the_continued_model(corpus_file):
    vocab, merges = hh.file_reference(corpus_file, 300)
    assert len(merges) == 300
    base = helpers.base_tokens(hh.SP)
    fresh = hh.fresh_flags(base, merges)
    # the bound at base + 150: a resumed stage 1, then stage 2 with the model's and stage 1's merges replayed
    want = hh.expected_stages(len(base), fresh, 220, len(base) + 150, n_old=80)
    assert want["id16_stages"] >= 1 and want["id16_merges"] >= 70 and want["id32_replayed_merges"] == 80 + want["id16_merges"] and want["id32_merges"] > 100
    # ... at base + 40 the model is past the bound already
    assert hh.expected_stages(len(base), fresh, 220, len(base) + 40, n_old=80) == stages(0, 0, 220, 80)
