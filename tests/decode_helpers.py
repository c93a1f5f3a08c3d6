"""Shared by the decoder tests: vocabs that stress BBPETokenizer.decode's id -> bytes rule, and id sequences over them."""
from __future__ import annotations

import random

from yet_another_bpe.tokenizer import BBPETokenizer

# one byte of every UTF-8 class (ASCII, continuation ranges, overlong / surrogate / out-of-range leads, never-valid bytes)
CLASS_BYTES = [0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1,
               0xF3, 0xF4, 0xF5, 0xFF]


def byte_tokenizer() -> BBPETokenizer:
    """The 256 single bytes, id = byte value: ids spell any byte string."""
    return BBPETokenizer(vocab={bytes([b]): b for b in range(256)}, merges=[])


def random_bytes(rng: random.Random, n: int) -> bytes:
    """Mostly class bytes and pieces of well-formed UTF-8, so that both repairs and intact characters are frequent."""
    out = bytearray()
    while len(out) < n:
        r = rng.random()
        if r < 0.4:
            out.append(rng.choice(CLASS_BYTES))
        elif r < 0.7:
            out += chr(rng.choice([0x41, 0xE9, 0x3B1, 0x4E2D, 0xFFFD, 0x1F600, 0x10FFFF, 0xD7FF, 0xE000])).encode("utf-8")
        else:
            out.append(rng.randrange(256))
    return bytes(out[:n])


def stress_tokenizers(rng: random.Random) -> list[tuple[str, BBPETokenizer]]:
    """Vocabs with every single byte plus multi-byte tokens (long ones too), id gaps, ids above 2^16, empty tokens and
    ids that two byte strings share (the last one in dict order wins)."""
    out = []
    for name in ("gaps", "duplicates", "empty", "wide_ids", "long_tokens"):
        vocab: dict[bytes, int] = {}
        ids = list(range(256))
        rng.shuffle(ids)
        for b, i in zip(range(256), ids):
            vocab[bytes([b])] = i * (3 if name == "gaps" else 1)
        nxt = max(vocab.values()) + 1
        for _ in range(300):
            t = random_bytes(rng, rng.randint(2, 8) if name != "long_tokens" else rng.randint(2, 300))
            if t in vocab:
                continue
            if name == "duplicates" and rng.random() < 0.4:
                vocab[t] = rng.choice(list(vocab.values()))
            elif name == "wide_ids":
                vocab[t] = rng.randrange(1 << 16, 1 << 20)
            else:
                vocab[t] = nxt
                nxt += rng.choice([1, 1, 2, 17]) if name == "gaps" else 1
        if name == "empty":
            vocab[b""] = nxt + 5
            vocab[b"x" * 3] = nxt + 5  # shares the empty token's id and wins (comes later)
            vocab[b""] = nxt + 6       # (re-assigning keeps the key's position: b"" stays first)
        out.append((name, BBPETokenizer(vocab=vocab, merges=[])))
    return out


def random_ids(rng: random.Random, tok: BBPETokenizer, n: int, unknown: float = 0.05) -> list[int]:
    """n ids of tok's vocab, with a share of ids it does not name (gaps, past the largest id)."""
    known = sorted(set(tok._vocab.values()))
    top = known[-1] if known else 0
    out = []
    for _ in range(n):
        if rng.random() < unknown:
            out.append(rng.choice([top + 1, top + 1000, rng.randrange(top + 2)]))
        else:
            out.append(rng.choice(known))
    return out
