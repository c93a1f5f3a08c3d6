"""Shared by the cl100k split-pattern tests: the pattern, the regex oracle for it, and the input lists (one case per rule of
csrc/split4_logic.h, special sets that lean on the reach of a special's end, whitespace and newline runs against the edges
of the kernels' 16-byte pieces and 4096-byte windows, runs longer than one iteration of the carry kernel, random strings)."""
from __future__ import annotations

import random

import regex

WIN = 4096        # PT_WIN of the kernels
PIECE = 16        # bytes per thread
CARRY = 2048      # windows per iteration of k_nl_carry
# whole-text lengths at which the shared scan code takes another path (tests/group_helpers.py)
TEXT_LENGTHS = (1, 15, 16, 17, WIN - 1, WIN, WIN + 1, CARRY * WIN, CARRY * WIN + 1)
GS = (1, 3, 255)


def pattern(G: int) -> str:
    return (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,%d}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+" % G)


_compiled: dict = {}


def regex_split(data: bytes, G: int, specials=(), chunk_starts=(0,)) -> list[bytes]:
    """regex.findall with the pattern, the specials in front of it in order; every chunk is a text of its own."""
    key = (G, tuple(specials))
    if key not in _compiled:
        pat = pattern(G)
        if specials:
            pat = "|".join(regex.escape(t) for t in specials) + "|" + pat
        _compiled[key] = regex.compile(pat)
    out: list[bytes] = []
    bounds = list(chunk_starts) + [len(data)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        out += [t.encode("utf-8") for t in _compiled[key].findall(data[a:b].decode("utf-8")) if t]
    return out


# one line per rule, then the cases the issue names
EDGE = [
    "a", "ab cd", "Hello, world!", "",
    # 1 contractions: every suffix, both cases, U+017F; what stands in front decides
    "it's", "I'M", "we'Ll", "they'RE", "you'vE", "he'd", "can't", "x'S", "x'ſ", "x'LL", "x'Re", "x'ſſ", "x'sx", "x'llx", "x'l", "x'v", "x'",
    "'s", "'ll", "\t's", " 's", "!'s", "\n's", "1's", "1'st", "a''s", "a's's", "a'ſ's", " 's", "a'S.b", "a's.b", "a'll.b", "a'ſ.b",
    "a's b", "a's  b", "a's\n", "a'ſ\n", "a'K", "a'ſt", "'", "''", "a'", "a' s",
    # 2 digits
    " 12", "1234567", "a1", "1a", " 1", "12 345", "١٢٣٤٥", "²³", "1²", "x1234567890y", "1.5", "1,234",
    # 3 letters and the one character in front
    ".a", "..a", " .a", "\ta", " a", "\na", "\ra", " a", "  a", "!a", "!!a", "a!b", "1.a", "…a", "……a", "😀a", "😀😀a", "a😀b", ".a.b", ". a", ".\ta",
    "　a", "\u001ca", "a　b", "a.b.c", "-a-b", "'a", "''a", "a'b",
    # 4 other
    "!", "!!", " !", "  !", "\t!", "a!", "1!", "! !", "!\t!", "a  !", "… …",
    # 5 newlines
    "a\n", "1\n", "!\n", "!\n\n", "!\r\n", " \n", "\n", "\n\n", "a\n\nb", "a \n b", "!\n a", "!\n\na", "! \n", "a\r\nb",
    # 6 whitespace, F and B
    "a b", "a  b", "a   b", "a  ", " ", "  ", "a \t b", "\n a", "\n  a", "\n \n a", "\n \n", "\n ", "\n  ", "!\n a", "!\n  a", "!\n\n  a", "!\n \n a",
    "!\n \n", "a\n \n", ".\n\n \nx", "\n\n \n x", "a\r\n  b", ".\n ", ".\n  ", ".\n \n", ".\n\t\n", "a\n\t", "a\n\t\tb", ".\r \r", " \n \n ", "\n \nx",
    "\n\u3000", ".\n\u3000x", ".\n\u3000 x", "a\n \n \n b", ".\n\n\n   \n\n  x", "x \n", "x  \n", "x  \n  ", "\t\n\t",
]

ALPHABET = (list("abXYslvLdmtTSeERſé") + ["'"] * 4 + list("0127²") + [" ", " ", " ", "\t", "\n", "\n", "\r", "\u00a0", "\u3000", "\u001c"]
            + list(".!…😀"))


def random_strings(seed: int, count: int, max_len: int = 24) -> list[str]:
    rng = random.Random(seed)
    return ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, max_len))) for _ in range(count)]


# special sets whose members meet the rules where a special ends or begins (none begins with \s or \p{N})
SPECIAL_SETS = [["<>"], ["<a>", ".x"], ["ab", "<"], ["'s", "e"], ["…", "😀a"], ["x!", "x"]]


def dense(specials, seed: int, count: int, max_len: int = 30) -> list[str]:
    """Random strings in which the specials, their prefixes and the alphabet alternate."""
    rng = random.Random(seed)
    pool = list(specials) * 3 + [t[:-1] for t in specials if len(t) > 1] + ALPHABET
    return ["".join(rng.choice(pool) for _ in range(rng.randint(1, max_len))) for _ in range(count)]


BEHIND_SPECIAL = ["<>…a", "<>😀a", "<>'s", "<>'ll.a", "<>'ſ.a", "<>.a", "<>..a", "<>\n a", "<>\n\n  a", "!<>\n a", "a<>a", "<><>", "<> a", "<>  a", "<>12345",
                  "<>\t's", "a'<>s", "!\n<>\n a", "!<>", "\n <>", "\n  <>x", "<>\n", ".<>\n\n x", "<\n >"]


def edge_runs() -> list[str]:
    """Whitespace and newline runs laid against every piece edge around a window edge, and against the window edge itself:
    the run starts k bytes in front of the edge and reaches past it; in front of it an O or a letter (B differs)."""
    out = []
    for k in range(0, 2 * PIECE + 2):
        for head in (".", "a"):
            for run, tail in (("\n" * 40, " x"), ("\n" + " " * 40, "\nx"), ("\n" + " " * 40, "x"), ("\n \n" * 14, " x"), ("\n" + "　" * 14, "x")):
                fill = "a" * (WIN - k - len(head.encode()))
                out.append(fill + head + run + tail)
    # whole windows of newlines / spaces with the cut exactly at a window's first and last byte
    out += ["." + "\n" * (WIN - 1) + " x", "." + "\n" * WIN + " x", "." + "\n" * (WIN - 2) + " x", "\n" + " " * (WIN - 1) + "\nx", "\n" + " " * (2 * WIN - 1) + "x",
            "a" * (WIN - 1) + "\n" + " " * WIN + "\n" + " " * WIN + "x", "a" * (WIN - 1) + "." + "\n" * (2 * WIN) + "  x"]
    return out


def long_runs() -> list[str]:
    """Runs of more than CARRY windows: the carry kernel takes a second iteration in both directions (about 8 MB each)."""
    n = (CARRY + 3) * WIN
    return ["." + "\n" * n + " x", "\n" + " " * n + "\n" + "x", "\n" + " " * n + "x"]


def chunk_cases() -> list[tuple[str, tuple]]:
    """Chunk starts inside whitespace and newline runs."""
    return [(".\n\n\n  x", (0, 2)), (".\n\n\n  x", (0, 1, 4)), ("\n   \n x", (0, 3)), ("\n   \n x", (0, 5)), ("a\n  \n  b", (0, 2, 3, 5)),
            (".\n x.\n x", (0, 4)), ("it's", (0, 2)), ("it's", (0, 3)), (".a.a", (0, 1)), ("..a", (0, 1)), ("12345678", (0, 4)),
            ("a" * (WIN - 2) + ".\n\n\n x", (0, WIN)), ("\n" + " " * (2 * WIN) + "\nx", (0, WIN + 1))]


def multilingual(golden_dir, n_bytes: int = 30_000) -> bytes:
    """The head of tests/golden/corpus.en with lines of other scripts, numbers, contractions in both cases, blank lines and
    indented lines between its lines."""
    rng = random.Random(41)
    lines = (golden_dir / "corpus.en").read_bytes()[:n_bytes].decode("utf-8", errors="ignore").split("\n")
    extra = ["Übergrößenträger … naïve café — «voilà»", "Привет, мир! Это тест 2024 года.", "こんにちは世界。１２３４５", "مرحبا بالعالم ١٢٣٤٥٦",
             "I'M sure THEY'LL say it's fine; we'Ve 12345 of them", "    indented\n\tand tabbed\r\n\r\n  x", "def f(x):\n    return x**2  # ok\n\n\n",
             "😀😀 emoji! 　wide space", "price: $1,234,567.89 on 12/31/1999", "x\n \n \n y", "", "", "   "]
    out = []
    for i, line in enumerate(lines):
        out.append(line)
        if i % 3 == 0:
            out.append(rng.choice(extra))
    return "\n".join(out).encode("utf-8")
