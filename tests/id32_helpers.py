"""Helpers of the u32-id tests (tests/test_gpu_id32.py, tests/test_gpu_id32_api.py): the synthetic model that fills the u16 id
space of tests/test_gpu_resume.py::test_id_space_exhausted_is_reported_not_truncated, and the corpus whose training crosses
65,534 tokens."""
from __future__ import annotations

import random
from functools import lru_cache

from tests import helpers

ID32 = {"id_bits": 32, "verify": 1}


@lru_cache(maxsize=None)
def crossing_model():
    """-> (base tokens, merges, words, freq): 65,526 tokens whose merges never touch the letters a, b, c, and 400 words over
    abc (random.Random(3)), pooled."""
    base = helpers.base_tokens([])
    letters = set(b"abc")
    pairs = [(bytes([x]), bytes([y])) for x in range(256) if x not in letters for y in range(256)]
    pairs += [(bytes([x]), bytes([y])) for x in letters for y in range(256) if y not in letters]
    merges = pairs[:65270]
    rng = random.Random(3)
    words = [bytes(rng.choice(b"abc") for _ in range(rng.randint(2, 12))) for _ in range(400)]
    words, freq = helpers.pooled(words)
    return base, merges, words, freq


@lru_cache(maxsize=None)
def api_corpus_words() -> tuple:
    """The words of the API tests' corpus, in file order (without the GPT-2 space prefix): random.Random(2), 20,000 draws of
    6 .. 14 letters, each repeated 1 .. 3 times."""
    rng = random.Random(2)
    out = []
    for _ in range(20_000):
        w = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(6, 14)))
        out += [w] * rng.randint(1, 3)
    return tuple(out)


def api_expected_words() -> list[bytes]:
    """What the GPT-2 pattern makes of the words joined by single spaces: every word but the first carries the space."""
    ws = api_corpus_words()
    return [ws[0]] + [b" " + w for w in ws[1:]]


def words_with_late_ids(tok, vocab, words, n: int) -> list[bytes]:
    """The first n corpus words (in file order, each once) whose encoding with the space prefix holds an id >= 65,536: the
    words that contain the bytes of such a token are encoded with the plain-Python tokenizer until n are found."""
    late = [t for t, i in vocab.items() if i >= 65_536]
    out = []
    for w in dict.fromkeys(words[1:]):
        sw = b" " + w
        if any(t in sw for t in late if len(t) <= len(sw)) and max(tok.encode(sw.decode())) >= 65_536:
            out.append(w)
            if len(out) == n:
                break
    return out
