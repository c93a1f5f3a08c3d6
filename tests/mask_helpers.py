"""Shared by the masked-language-model tests, CPU and GPU: a small tokenizer over the golden corpus.en model with specials
that include [MASK], [PAD] and one special without an id, the texts the word-index tests encode, and the synthetic ids with
document lengths from lists that the mask tests run on (no tokenizer model is needed there)."""
from __future__ import annotations

import json
from functools import lru_cache
from pathlib import Path

import numpy as np

from tests import helpers
from yet_another_bpe.tokenizer import BBPETokenizer

GOLDEN = Path(__file__).resolve().parent / "golden"
NO_ID = "<|noid|>"  # a special the vocab lacks: it takes a piece index and emits nothing
SPECIALS = ["<|endoftext|>", "[MASK]", "[PAD]", NO_ID]
SPECIALS_LOWER = ["<|endoftext|>", "[mask]", "[pad]", NO_ID]  # (a lowercase model matches its specials in the lowered text)
IGNORE = -100


@lru_cache(maxsize=None)
def _model():
    vocab = {bytes.fromhex(k): v for k, v in json.loads((GOLDEN / "g1_corpus_en_vocab_1000.json").read_text()).items()}
    return vocab, helpers.read_hex_merges(GOLDEN / "g1_corpus_en_exhaustive.hex")[:743]


def tokenizer(specials=SPECIALS, **options) -> BBPETokenizer:
    """The corpus.en model of tests/encode_helpers.py (vocab 1000, 743 merges) with `specials`, each but NO_ID with an id."""
    vocab, merges = _model()
    vocab = dict(vocab)
    for s in specials:
        if s != NO_ID and s.encode() not in vocab:
            vocab[s.encode()] = max(vocab.values()) + 1
    return BBPETokenizer(vocab=vocab, merges=list(merges), special_tokens=list(specials), **options)


@lru_cache(maxsize=None)
def corpus_words() -> tuple[str, ...]:
    return tuple((GOLDEN / "corpus.en").read_text(encoding="utf-8").split())


def word_docs(mask: str = "[MASK]") -> list[str]:
    """Empty documents; specials only; the special without an id; a 90-byte pre-token (the sequential path) and one of 45
    two-byte letters; one document of about 700 pre-tokens (more than a block of 256); 300 short documents (many documents
    in a block), some of them empty; an empty document at the end."""
    words = corpus_words()
    long_doc = " ".join(words[(7 * i) % len(words)] for i in range(700))
    short = [("" if i % 11 == 5 else f"{words[i % len(words)]} it's {i * 7}.") for i in range(300)]
    return (["", "", f"<|endoftext|>{mask}<|endoftext|>", f"a {NO_ID} b{NO_ID}{NO_ID}c 12345 {mask}x", NO_ID, "x" * 90 + " tail " + "é" * 45,
             long_doc, ""] + short + [f"{NO_ID}<|endoftext|>", ""])


# one text each for the plain-Python contract under the tokenizer's options
OPTION_TEXTS = [
    ({"digit_group": 3}, SPECIALS, f"In 1234567 we paid 89012.50<|endoftext|>{NO_ID} 007"),
    ({"pretokenizer": "cl100k"}, SPECIALS, f"It'S 12345 o'clock\n\n  [MASK]done {NO_ID}\r\n x"),
    ({"pretokenizer": "o200k_base"}, SPECIALS, f"CamelCaseWord it's 98765 HTTPServer{NO_ID}[PAD] naïve"),
    ({"lowercase": True}, SPECIALS_LOWER, f"Hello WORLD İstanbul [mask] {NO_ID}Done"),
    ({"normalizer": "nfc"}, SPECIALS, f"naïve café [MASK]{NO_ID} éé"),
]
# the option sets of the GPU word-index test (the last one: lowercase plus "nfc")
GPU_OPTIONS = [({"digit_group": 3}, SPECIALS, "[MASK]"), ({"pretokenizer": "cl100k"}, SPECIALS, "[MASK]"),
               ({"pretokenizer": "o200k_base"}, SPECIALS, "[MASK]"), ({"lowercase": True, "normalizer": "nfc"}, SPECIALS_LOWER, "[mask]")]

# ---------------------------------------------------------------- synthetic ids for the mask rule
# document lengths: (name, lengths, doc_off given) -- a kernel block is 256 ids
LENGTH_SETS = [
    ("empty documents at the start, the middle and the end", [0, 0, 5, 0, 0, 7, 300, 0, 3, 0, 0], True),
    ("600 one-token documents", [1] * 600, True),
    ("one 700-token document next to 3-token ones", [3, 3, 700, 3, 3], True),
    ("no ids", [0, 0, 0], True),
    ("one document, no ids", [0], True),
    ("one document without doc_off", [77], False),
    ("one document over three blocks without doc_off", [515], False),
    ("a block boundary at a document boundary", [256, 256, 1], True),
    ("mixed", np.random.default_rng(9).integers(0, 40, 120).tolist(), True),
]


def synth_batch(lens, seed: int = 1):
    """-> (ids_batch, words_batch, special_batch) for documents of the given lengths: ids below 1000, piece indices that
    never decrease (steps of 0, 1, 2: pieces of several ids and gaps), one id in sixteen a special occurrence."""
    rng = np.random.default_rng(seed)
    ids, words, special = [], [], []
    for n in lens:
        ids.append(rng.integers(0, 1000, n).tolist())
        words.append((np.cumsum(rng.integers(0, 3, n)) if n else np.zeros(0, np.int64)).tolist())
        special.append((rng.integers(0, 16, n) == 0).tolist())
    return ids, words, special


def flat(batch, dtype) -> np.ndarray:
    return np.asarray([x for doc in batch for x in doc], dtype=dtype)


def starts(lens) -> np.ndarray:
    """the n_docs document starts as u64 (the table the C ABI takes)"""
    s = np.zeros(max(len(lens), 1), dtype=np.uint64)
    s[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))[:-1]
    return s


def packed_words(words_batch, special_batch) -> np.ndarray:
    """words | special << 31: what yabpe_encode_words returns and yabpe_mask reads"""
    return flat(words_batch, np.uint32) | (flat(special_batch, bool).astype(np.uint32) << 31)


def kinds(ids_batch, inputs, labels, special_batch, mask_id):
    """-> per document, per token: "protected", "unselected", "masked", "random" or "kept" -- read off a mask_tokens result.
    Exact when the batch holds neither mask_id nor an id below n_random (a random id then differs from the original)."""
    out = []
    for d, ids in enumerate(ids_batch):
        row = []
        for j, tid in enumerate(ids):
            if labels[d][j] == IGNORE:
                row.append("protected" if special_batch is not None and special_batch[d][j] else "unselected")
            elif inputs[d][j] == mask_id:
                row.append("masked")
            elif inputs[d][j] == tid:
                row.append("kept")
            else:
                row.append("random")
        out.append(row)
    return out
