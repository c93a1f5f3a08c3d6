"""Inputs and CPU references of the u32 resumed-load and hand-over tests (tests/test_gpu_id32_resume.py,
tests/test_gpu_id32_handover.py).  Nothing here touches a GPU: the recipes are deterministic
(random.Random with fixed seeds), the references are the C oracle, tie_helpers.replay, limit_helpers.train and the literal
replay of resume_helpers.  tests/test_id32_handover_inputs.py asserts, from these alone, every condition the GPU tests rely
on, so a changed recipe fails on the CPU."""
from __future__ import annotations

import random
from functools import lru_cache
from pathlib import Path

from oracle import oracle
from tests import helpers, limit_helpers as lh, resume_helpers as rh, tie_helpers

SP = ["<|endoftext|>"]
LONG = 64  # tokens from which a word leaves the u32 tile stream (csrc/yabpe_id32_kernels.h: LMAX32)


# ================================================================ the stage arithmetic of BBPETrainer._run
def fresh_flags(base, merges) -> list[bool]:
    """Per merge: its bytes are a new token (False: a token already, the merge reuses that id)."""
    known, out = set(base), []
    for left, right in merges:
        out.append(left + right not in known)
        known.add(left + right)
    return out


def expected_stages(n_base: int, fresh, budget: int, u16: int, n_old: int = 0, mode: str = "auto") -> dict | None:
    """What _run's last_stats must say, from a reference merge list alone.  `fresh`: fresh_flags of the reference's merges, the
    first n_old being the model's (train_from), the rest what a budget of `budget` iterations learns (fewer: a stop rule
    ended the job); `u16`: the patched trainer.U16_TOKENS.  The rule: the u16 path is asked for min(budget left, ids left)
    merges while that is positive, a call that returns fewer ends the job, the u32 path replays everything so far and runs
    the rest.  None: the job fits below the bound and takes the old route (no id16_* / id32_* entries)."""
    n_tokens = n_base + sum(fresh[:n_old])
    new = list(fresh[n_old:])
    assert len(new) <= budget
    if mode == "auto" and n_tokens + budget <= u16:
        return None
    n_done = stages = 0
    stopped = False
    while mode == "auto" and not stopped:
        ask = max(0, min(budget - n_done, u16 - n_tokens))
        if not ask:
            break
        got = new[n_done:n_done + ask]
        n_tokens += sum(got)
        n_done += len(got)
        stages += 1
        stopped = len(got) < ask
    out = {"id16_merges": n_done, "id16_stages": stages, "id32_merges": 0, "id32_replayed_merges": 0}
    if not stopped and n_done < budget:
        out.update(id32_merges=len(new) - n_done, id32_replayed_merges=n_old + n_done)
    return out


def picked(stats: dict) -> dict:
    return {k: stats[k] for k in ("id16_merges", "id16_stages", "id32_merges", "id32_replayed_merges")}


# ================================================================ A2: small tie-heavy corpora with specials
@lru_cache(maxsize=None)
def random_small(seed: int = 9417, n: int = 40) -> tuple:
    """The recipe of test_random_small_vs_oracle: -> ((words, specials, vocab_size, min_frequency, oracle vocab, oracle merges), ...)"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        al = rng.choice([b"ab", b"abc", b"xyz ", bytes([0, 255, 254, 1]), b"abcdefghijklmnop"])
        words = []
        for _ in range(rng.randint(1, 40)):
            words += [bytes(rng.choice(al) for _ in range(rng.randint(1, 30)))] * rng.randint(1, 6)
        rng.shuffle(words)
        sp = rng.choice([[], ["ab"], ["<|x|>"], ["a", "b"], ["[PAD]", "[UNK]", "[BOS]", "[EOS]"]])
        vs, mf = 256 + rng.randint(0, 120), rng.randint(1, 3)
        vocab, merges = oracle.merge_loop(words, vs, mf, sp)
        out.append((tuple(words), tuple(sp), vs, mf, vocab, merges))
    return tuple(out)


# ================================================================ A3 / B2 / B7: reused ids
@lru_cache(maxsize=None)
def reuse_case(name: str) -> dict:
    """A case of tie_helpers.reuse_cases with its references: `hits` (tie_helpers.replay: the merges whose bytes were a token
    already), the oracle's model on the occurrences at the budget of tests/test_gpu_id32.py (200 merges past the specials)."""
    _n, types, freqs, specials = next(c for c in tie_helpers.reuse_cases() if c[0] == name)
    steps = tie_helpers.replay(types, freqs, specials)
    words = [w for w, f in zip(types, freqs) for _ in range(f)]
    base = helpers.base_tokens(specials)
    vocab_size = 256 + len(specials) + 200
    vocab, merges = oracle.merge_loop(words, vocab_size, 1, list(specials))
    return {"types": list(types), "freqs": list(freqs), "specials": list(specials), "base": base, "vocab_size": vocab_size,
            "budget": vocab_size - len(base), "hits": [k for k, s in enumerate(steps) if s["hit"]], "n_steps": len(steps),
            "pairs": [s["pair"] for s in steps], "vocab": vocab, "merges": merges}


def reuse_splits(case: dict) -> list[int]:
    """Directly before and directly after every hit, and once past the last one"""
    hits = case["hits"]
    return sorted({k for h in hits for k in (h, h + 1)} | {min(hits[-1] + 5, len(case["merges"]) - 1)})


# ================================================================ A3b: a merge that must not apply after its rank has passed
def per_word_replay(word: bytes, merges, rank_floor: bool = True, leftmost: bool = True) -> tuple:
    """The per-word form of the replay as the load kernels run it, in plain Python: again and again the leftmost adjacent pair
    whose smallest rank >= t is the minimum over the word merges, and t follows.  With both flags it equals
    resume_helpers.literal_replay; the flags switch off one rule each, to show that an input tells the rule from its absence."""
    ranks: dict = {}
    for k, pair in enumerate(merges):
        ranks.setdefault(pair, []).append(k)
    w, t = [bytes([b]) for b in word], 0
    while len(w) > 1:
        best = None
        for p in range(len(w) - 1):
            r = next((k for k in ranks.get((w[p], w[p + 1]), ()) if k >= t or not rank_floor), None)
            if r is not None and (best is None or r < best[0] or (r == best[0] and not leftmost)):
                best = (r, p)
        if best is None:
            break
        t, p = best
        w[p:p + 2] = [w[p] + w[p + 1]]
    return tuple(w)


def late_operand_case() -> dict:
    """A model whose FIRST merge names a token that the words only hold after the LAST one: (abc, d) with the special "abc",
    then (a, b) and (ab, c), which reuses the special's id.  In the training loop (abc, d) met no pair, so the literal replay
    leaves "abc d"; a replay that forgets which rank it has passed merges it.  (A model like this comes from a corpus where
    "abc" stood as another split, or from anyone who writes merges by hand: train_from replays them as they are.)"""
    specials = ["abc"]
    base = helpers.base_tokens(specials)
    merges = [(b"abc", b"d"), (b"a", b"b"), (b"ab", b"c")]
    words = [b"abcd", b"abcdabcd", b"xabcd", b"abc", b"dabc", b"abcabcd", b"dd"]
    freqs = [7, 5, 4, 3, 3, 2, 2]
    vocab, all_merges = rh.resume_naive([w for w, f in zip(words, freqs) for _ in range(f)], base, merges, 12, 1)
    return {"specials": specials, "base": base, "merges": merges, "words": words, "freqs": freqs, "budget": 12,
            "vocab": vocab, "all_merges": all_merges}


# ================================================================ A4: long words
@lru_cache(maxsize=None)
def long_words() -> tuple:
    """The words of tests/test_gpu_id32.py::test_long_words"""
    rng = random.Random(77)
    words = [bytes(rng.choice(b"abcdefgh") for _ in range(n)) for n in (64, 65, 100, 129, 200, 257, 300)]
    words += [b"z" * 500, b"q" * 62, b"q" * 63, b"q" * 64, b"ab" * 31 + b"a", b"ab" * 32]
    words += [b"abcabc"] * 7 + [b"aaa", b"zz"]
    return tuple(words)


LONG_SPLITS = (0, 3, 5, 12, 40, 150)


@lru_cache(maxsize=None)
def long_reference():
    """(vocab, merges) of the oracle on long_words() at 150 + 150 merges"""
    return oracle.merge_loop(list(long_words()), 257 + 300, 1, SP)


def long_lengths(k: int) -> dict[bytes, int]:
    """{word type: its tokens after the literal replay of the reference's first k merges}"""
    merges = long_reference()[1][:k]
    return {w: len(rh.literal_replay(w, merges)) for w in dict.fromkeys(long_words())}


# ================================================================ A5: a new corpus
def synth_words(spec) -> list[bytes]:
    from yet_another_bpe import synth

    flat, off = synth.generate(spec)
    fb, o = flat.tobytes(), off.tolist()
    return [fb[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def new_corpus_specs():
    """test_new_corpus_equals_the_naive_continuation at a quarter of its size: (spec A, spec B, merges on A, merges on B)"""
    from yet_another_bpe import synth

    return (synth.SynthSpec(75 << 10, 1000, 5, b"abcdefghijklmnopqrstuvwxyz", True),
            synth.SynthSpec(75 << 10, 750, 77, b"aeioubcdxyz0123456789-", True), 150, 90)


@lru_cache(maxsize=None)
def new_corpus():
    """-> (words A, words B, the oracle's model on A (vocab, merges), the naive continuation on B (vocab, all merges))"""
    spec_a, spec_b, n_a, n_b = new_corpus_specs()
    words_a, words_b = synth_words(spec_a), synth_words(spec_b)
    model = oracle.merge_loop(words_a, 257 + n_a, 2, SP)
    want = rh.resume_naive(words_b, helpers.base_tokens(SP), model[1], n_b, 2)
    return words_a, words_b, model, want


# ================================================================ A7: a maximum token length after a replay
LIMIT_MODEL_MERGES, LIMIT_MORE = 200, 150


@lru_cache(maxsize=None)
def limit_model():
    """(pooled words, counts, merges) of limit_helpers.train without a limit on the 6,000 pre-tokens of corpus.en"""
    uw, fq = helpers.pooled(lh.en_words())
    _vocab, merges = lh.train(uw, fq, LIMIT_MODEL_MERGES, 1, SP, limit=None)
    return uw, fq, merges


@lru_cache(maxsize=None)
def limit_continuation(limit: int):
    """(vocab, all merges): the model's merges replayed whatever their length, then LIMIT_MORE merges that skip the pairs over `limit`"""
    uw, fq, model = limit_model()
    vocab, new = lh.train(uw, fq, LIMIT_MORE, 1, SP, limit=limit, start_merges=model)
    return vocab, list(model) + new


@lru_cache(maxsize=None)
def limit4_reference():
    """(vocab, merges) of limit_helpers.train with a limit of 4 bytes at 300 merges (B4)"""
    uw, fq = helpers.pooled(lh.en_words())
    return lh.train(uw, fq, 300, 1, SP, limit=4)


# ================================================================ B1 / B3: the tie-heavy corpora at the words level
TIE_BUDGET = 400


@lru_cache(maxsize=None)
def tie_reference(name: str):
    """(types, freqs, the oracle's (vocab, merges) on the occurrences) of tie_helpers.<name> at 400 merges, no specials"""
    types, freqs = getattr(tie_helpers, name + "_types")()
    return list(types), list(freqs), oracle.merge_loop(getattr(tie_helpers, name)(), 256 + TIE_BUDGET, 1, [])


@lru_cache(maxsize=None)
def stop_points() -> dict:
    """The stop-rule cases on `stems`, from the counts of tie_helpers.replay (the best count never rises, so a min_frequency
    of counts[j - 1] > counts[j] ends the job after exactly j merges):
      early   (min_frequency, j, h): j < h, the job ends inside stage 1
      seam    (min_frequency, j, h): j = h + 1, the job ends after exactly one merge of stage 2"""
    types, freqs = tie_helpers.stems_types()
    counts = [s["count"] for s in tie_helpers.replay(types, freqs, (), num_merges=60)]
    drops = [j for j in range(1, len(counts)) if counts[j] < counts[j - 1]]
    early = next(j for j in drops if j >= 3)
    seam = next(j for j in drops if j >= early + 8)
    return {"counts": counts, "early": (counts[early - 1], early, early + 6), "seam": (counts[seam - 1], seam, seam - 1)}


# ================================================================ B5 / B6 / B7: a corpus file
FILE_CFG = dict(min_frequency=1, max_workers=1, chunk_size_bytes=4 << 10, special_tokens=SP)
FILE_CASES = {"gpt2_g3": dict(pretokenizer="gpt2", digit_group=3), "cl100k": dict(pretokenizer="cl100k"),
              "o200k_base": dict(pretokenizer="o200k_base"), "cl100k_nfc": dict(pretokenizer="cl100k", normalizer="nfc")}
FILE_MERGES, FILE_H = 200, 60
EXTRAS = ("don't", "I'LL", "we've", "it's", "HTTPServer", "fooBar", "XMLParser", "cafe\u0301", "nai\u0308ve", "1234567", "42",
          "2024", "3.14159", "x86")


@lru_cache(maxsize=None)
def file_text() -> str:
    """About 40 KiB: 60 documents of 60 .. 140 words drawn from a lexicon of a few hundred syllable words (random.Random(2024),
    a heavy-tailed rank), every eighth word or so one of EXTRAS (digit runs, contractions in either case, mixed case,
    combining sequences), some capitalised, with commas, full stops and line breaks, joined by the special token."""
    rng = random.Random(2024)
    syll = ["ba", "ne", "ti", "ro", "ku", "sha", "lem", "or", "in", "est", "un", "ply", "gra", "ve", "do", "mi"]
    lex = list(dict.fromkeys("".join(rng.choice(syll) for _ in range(rng.randint(1, 4))) for _ in range(400)))
    docs = []
    for _ in range(60):
        parts = []
        for _ in range(rng.randint(60, 140)):
            w = rng.choice(EXTRAS) if rng.random() < 0.12 else lex[min(int(rng.paretovariate(0.7)) - 1, len(lex) - 1)]
            if rng.random() < 0.08:
                w = w.capitalize()
            parts.append(w + rng.choice(["", "", "", "", ",", ".", ".\n", "\n\n"]))
        docs.append(" ".join(parts))
    return SP[0].join(docs) + "\n"


def write_file(path: Path) -> Path:
    path.write_bytes(file_text().encode("utf-8"))
    return path


def file_words(path: Path, **config) -> list[bytes]:
    """The file's pre-tokens by the trainer's own plain-Python _pretokenize (normalize_text first where a normaliser is set)"""
    from yet_another_bpe.trainer import BBPETrainer, BBPETrainerConfig

    t = BBPETrainer(BBPETrainerConfig(**{**FILE_CFG, **config}))
    return [s.encode("utf-8") for s in t._pretokenize([path])]


_file_models: dict = {}


def file_reference(path: Path, n_merges: int = FILE_MERGES, **config):
    """(vocab, merges) of the oracle over file_words at n_merges (computed once per configuration)"""
    key = (n_merges, tuple(sorted(config.items())))
    if key not in _file_models:
        _file_models[key] = oracle.merge_loop(file_words(path, **config), 257 + n_merges, 1, SP)
    return _file_models[key]
