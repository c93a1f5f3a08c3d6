"""CPU: the device encoder's BPE-dropout rules (yet-another-bpe_amd/csrc/encode_logic.h: keys, draws, the sequential walk with
its set-aside entries, and the every-candidate-draws rule of the lane form) id for id against BBPETokenizer.encode_dropout --
on the G9 set-ups (the lossy from_file reload and the vocabs lacking bytes among them) and on random tie-heavy models with
duplicate merges; pre-tokens of every length at which the device changes its path, multi-byte text, specials, empty documents."""
from __future__ import annotations

import random

import pytest

from tests import dropout_helpers as dh
from tests import encode_helpers

PS = [0.0, 0.1, 0.5, 0.9, 1.0]
SEEDS = [0, 12345, (1 << 64) - 1]


@pytest.fixture(scope="module")
def model():
    return dh.load_model()


def check(lib, tok, docs, p, seed, what):
    T = tok._dropout_threshold(p)
    got, err = dh.model_encode(lib, tok, [d.encode("utf-8") for d in docs], T, seed)
    assert err == -1
    exp = tok.encode_batch_dropout(docs, p, seed)
    assert got == exp, (what, p, seed, next(d for d in range(len(docs)) if got[d] != exp[d]))
    if p == 0.0:
        assert got == tok.encode_batch(docs), what
    if p == 1.0:
        assert got == [dh.per_byte(tok, d) for d in docs], what
    return got


def test_g9_setups_every_p_and_seed(model, golden_dir, tmp_path):
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    assert {"from_file", "in_memory", "lacking_bytes_with_unk", "lacking_bytes_no_unk"} <= {name for _i, name, _t in setups}
    for k, (_idx, name, tok) in enumerate(setups):
        docs = dh.documents(tok.special_tokens)
        full = name == "in_memory"
        for j, p in enumerate(PS):
            for seed in SEEDS if full else [SEEDS[(j + k) % 3]]:
                check(model, tok, docs, p, seed, name)


def test_specials_with_and_without_id(model, golden_dir, tmp_path):
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    tok = dh.with_specials(next(t for _i, name, t in setups if name == "in_memory"))
    docs = dh.documents([dh.SP, dh.SP_NOID])
    for p in PS:
        for seed in SEEDS:
            got = check(model, tok, docs, p, seed, "specials")
            assert got[0] != got[2] or p in (0.0, 1.0)  # equal documents, different draws


def test_random_tie_heavy_models(model):
    rng = random.Random(9)
    for trial in range(60):
        alphabet = rng.choice(["ab", "abc", "a b", "xy'", "ab\n"])
        specials = rng.choice([[], ["<s>"], ["ab", "a"], ["aa"], [" b"]])
        tok = encode_helpers.random_model(rng, alphabet, rng.randint(1, 40), specials, drop_bytes=rng.random() < 0.4,
                                          with_unk=rng.random() < 0.5)
        texts = ["".join(rng.choice(alphabet + "a") for _ in range(rng.randint(0, 30))) for _ in range(12)]
        texts += ["", "a" * rng.randint(1, 80), "ab" * rng.randint(1, 40), " " + "b" * rng.randint(60, 90), "ab" * 150]
        check(model, tok, texts, rng.choice(PS), rng.choice(SEEDS), (trial, alphabet, specials))
