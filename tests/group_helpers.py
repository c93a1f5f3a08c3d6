"""Shared by the digit-group tests: the grouped split pattern, the regex oracle for it, and the input lists (hand-written
digit cases, strings whose digit runs meet the edges of the kernel's 4096-byte windows, random strings)."""
from __future__ import annotations

import random

import regex

from tests.test_pretok_model import EDGE

WIN = 4096  # GRP_WIN / PT_WIN of the kernels
# Whole-text lengths at which the shared scan code (csrc/yabpe_scan_kernels.h) takes another path: the guarded tail of the piece
# load and store, the last window, and exactly one tile of 2,048 windows of the carry kernels, and one window more.
TEXT_LENGTHS = (1, 15, 16, 17, WIN - 1, WIN, WIN + 1, 2048 * WIN, 2048 * WIN + 1)


def grouped_pattern(G: int) -> str:
    """The GPT-2 pattern with \\p{N}+ replaced by \\p{N}{1,G} (G = 0: unchanged)."""
    digits = r"\p{N}+" if not G else r"\p{N}{1,%d}" % G
    return r"""'(?:[sdmt]|ll|ve|re)| ?\p{L}+| ?""" + digits + r"""| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""


def regex_split(data: bytes, G: int, specials=(), chunk_starts=(0,)) -> list[bytes]:
    """regex.findall with the grouped pattern, the specials in front of it in order; every chunk is a text of its own."""
    pat = grouped_pattern(G)
    if specials:
        pat = "|".join(regex.escape(t) for t in specials) + "|" + pat
    pat = regex.compile(pat)
    out: list[bytes] = []
    bounds = list(chunk_starts) + [len(data)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        out += [t.encode("utf-8") for t in pat.findall(data[a:b].decode("utf-8")) if t]
    return out


DIGITS = ["1234567", " 1234", "  1234", "a1234b", "12's", "1,234.5678", "١٢٣٤٥", "²³½Ⅷ12", "12\n345", "1", "12", "123", "1234", " 1", " 12 123 1234 12345",
          "1 2", "12 ١٢٣٤ 56", "x123456789y", "3.14159", "'s12345", "1's2345", "\t12345", " \n12345", "12345 ", "१२३४५६७", "a١b٢٣٤c", "½½½½½½½"]
# specials that contain or end with digits but do not begin with one; two digits in a row inside a special and a special
# that is a space and digits must not be cut
SPECIALS = [[], ["<x1"], ["<|7|>"], ["s1"], ["<|e|>", "<x1"], ["<x12", " 12"], ["<|endoftext|>"], [" <s>"], ["<1234567>"]]
SPECIAL_TEXTS = ["<x1234", "<x12345678", "a<x1", "<x1<x1", "<|7|>777", "7<|7|>7", "1234<|7|>5678", "s1234", "ss12345", "s1s1s1", "12s123",
                 "<|e|>1234<x1234", "<x123456", "a 1234", " 12 12", " 123456", "x 12<x12345", "<|endoftext|>12345<|endoftext|>", "12345 <s>6789",
                 "<1234567>1234567", "<1234567", "s1's12", "1s1234"]


def window_cases(word: str = "a") -> list[str]:
    """Digit runs against the window edges: a run of 3 windows and a few bytes, a run that starts on the last byte of a
    window, a multi-byte digit across an edge, windows made of continuing digits only (with a start exactly at a window's
    first byte and without).  The text in front of a run is `word` repeated (ASCII), cut to the length wanted."""
    class Fill:
        def __mul__(self, k):
            return (word * (k // len(word) + 1))[:k]

    a = Fill()
    return [
        "1" * (3 * WIN + 5),
        a * (WIN - 1) + "123456789",
        a * (WIN - 2) + "1" + "٣" + "٣٣٣٣" + "12",       # the two bytes of the second digit are WIN - 1 and WIN
        a * (WIN - 3) + "1" + "१" + "234567",            # a three-byte digit: WIN - 2 .. WIN
        a * WIN + "7" * (2 * WIN + 9),                   # a start exactly at a window's first byte, then two full windows
        a * (WIN - 6) + "7" * (2 * WIN + 17),            # no start in windows 1 and 2
        " " + "٣" * (WIN + 100),                           # multi-byte digits only, the space in front
        "12 " * (WIN // 3 + 10) + "9" * (WIN + 1),
    ]


ALPHABETS = ["0123456789", "12 ", "1a ", "1٣²½ a\n", "12's 'll", "1 　\n2", "<|>-x1e7s", "123 <x1s", "١٢٣12 '", "1.,2"]


def random_strings(seed: int, count: int, max_len: int = 40) -> list[str]:
    rng = random.Random(seed)
    return ["".join(rng.choice(al) for _ in range(rng.randint(1, max_len))) for al in (rng.choice(ALPHABETS) for _ in range(count))]


def leads_with_digit(token: str) -> bool:
    return bool(regex.match(r"\p{N}", token))


ALL_EDGE = [s for s in EDGE + DIGITS + SPECIAL_TEXTS if s]


def number_corpus(golden_dir, n_bytes: int = 40_000) -> bytes:
    """The head of tests/golden/corpus.en with number-heavy lines between its lines: prices, dates, long digit runs, digits
    of other scripts, digits next to letters and specials' look-alikes."""
    rng = random.Random(23)
    lines = (golden_dir / "corpus.en").read_bytes()[:n_bytes].decode("utf-8", errors="ignore").split("\n")
    out = []
    for i, line in enumerate(lines):
        out.append(line)
        if i % 3 == 0:
            k = rng.randrange(6)
            out.append([f"In {rng.randrange(1000, 2100)} the total was {rng.randrange(10 ** 7):,} or {rng.random() * 1000:.4f} units.",
                        f"call {rng.randrange(10 ** 10):010d} before {rng.randrange(1, 13)}/{rng.randrange(1, 29)}/{rng.randrange(1990, 2030)}",
                        "pi = 3.14159265358979323846264338327950288419716939937510",
                        f"id{rng.randrange(10 ** 5)}x{rng.randrange(10 ** 12)} ١٢٣٤٥٦ २०२४ ²³ ½",
                        f"  {rng.randrange(10 ** 4)}  {rng.randrange(10 ** 6)}\t{rng.randrange(10 ** 9)}",
                        f"it's 12's and 1234's, v{rng.randrange(10)}.{rng.randrange(100)}.{rng.randrange(1000)}"][k])
    return "\n".join(out).encode("utf-8")


def digits_in(token: bytes) -> int:
    return len(regex.findall(r"\p{N}", token.decode("utf-8", errors="ignore")))
