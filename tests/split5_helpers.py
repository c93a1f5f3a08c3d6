"""Shared by the o200k_base split-pattern tests: the pattern, the regex oracle for it, and the input lists (a case per
transition of the scanner in csrc/split5_logic.h, special sets dense in the text, chunk starts inside runs, runs against
the edges of the kernels' 16-byte pieces and 4096-byte windows, chains longer than one iteration of the carry kernels,
random strings)."""
from __future__ import annotations

import random

import regex

WIN = 4096        # PT_WIN of the kernels
PIECE = 16        # bytes per thread
CARRY = 2048      # windows per iteration of k_la_carry / k_fn_carry
# whole-text lengths at which the shared scan code takes another path (tests/group_helpers.py)
TEXT_LENGTHS = (1, 15, 16, 17, WIN - 1, WIN, WIN + 1, CARRY * WIN, CARRY * WIN + 1)
GS = (1, 3, 255)

_SUFFIX = r"(?i:'s|'t|'re|'ve|'m|'ll|'d)?"


def pattern(G: int) -> str:
    return (r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+" + _SUFFIX
            + r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*" + _SUFFIX
            + r"|\p{N}{1,%d}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+" % G)


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


def offsets(words: list[bytes]) -> list[int]:
    out = [0]
    for w in words:
        out.append(out[-1] + len(w))
    return out


M = "́"  # a \p{M} character
# the cases the issue names, then a line per state of the scanner: what keeps it, what leaves it
EDGE = [
    "", "a", "A", "Hello, world!",
    "HTTPServer fooBar FOObarBAZ", "ABCアDE", "!" + M + "a", "!!" + M + "a", M + "!a", "!\n/a", "ab's's's", "don'tknow 'tis",
    # S0: every class at a boundary, the prefix character, " ?" of the punctuation, the three whitespace rules
    "aA", "Aa", "ア", M, "ʰ", "ǅ", "ǅa", "1", "²", " a", " A", " ア", " " + M, "\ta", " a", "　A", "!a", "!A", "'a", "/a", "\na", "\ra", " 1", "!1",
    " !", " !!", " …", "  !", "\t!", " !", " /", " \n", " \r", "\n", "\r\n", "\n\n", " \n\n", "  \n", " \t\n x", " ", "  ", "   ", " \t", "\t ", "a ", "a  ", "a   ",
    "a  b", "a   b", "a \t b", "  a", "   a", " \t1", "  1", "  !", "   !", "a　　b",
    # WSR: up to the run's last R; what follows it starts anew
    "\n a", "\n  a", "\n \n a", "\n \n", "\n ", "\n  ", " \n \n ", "\n \nx", "\n\n \n x", "a\n \n \n b", "x \n", "x  \n  ", "\t\n\t", "\n　", "\r \r", "\n\n  \n\n  x", "\n!",
    "\n1", "\n\n\n", "a\n\nb", "a\r\nb", " \n!", "\n !", "\n  !", "\n \n!",
    # WSP: the last whitespace in front of a non-space
    "a  !", "a  1", "a   1", "a \t b", "   　", "a  " + M,
    # PFX and the three word states
    "!ab", "!Ab", "!AB", "!" + M, "!" + M + M, " " + M + "a", "!ア", "!ʰ", " ǅ", "aB", "aBc", "aBC", "ABc", "ABCd", "ABCDe", "ABC", "ABC ", "ABC!", "ABC1", "AB\n",
    "aアB", "AアB", "AアBc", "Aアb", "AアBC", "Aア", "Aア ", "AアBCアd", "AアBア", "AアBアc", "A" + M + "B", "A" + M + "Bc", "a" + M + "B", "A" + M + "b" + M + "C",
    "aʰB", "AʰB", "AʰBc", "ǅB", "ǅBc", "ǅb", "AǅB", "aǅb", "アA", "アAb", "アAB", "アa", "アaB", M + "A", M + "Ab", M + "a", "ʰAb",
    "camelCaseWord", "XMLHttpRequest", "iPhone", "McDonald", "ÉCOLE", "école", "ÉcoleNormale", "ΑΒΓαβγ", "ПриветМИР", "こんにちはABCdef",
    # contractions: a suffix of the word; every suffix, both cases, U+017F; what stands in front and behind
    "it's", "I'M", "we'Ll", "they'RE", "you'vE", "he'd", "can't", "x'S", "x'ſ", "x'LL", "x'Re", "x'ſſ", "x'sx", "x'llx", "x'l", "x'v", "x'", "X'S", "X'sx", "X'Sx", "XY'llZ",
    "'s", "'ll", "\t's", " 's", "!'s", "\n's", "1's", "1'st", "a''s", "a's's", "a'ſ's", "a'S.b", "a's.b", "a'll.b", "a's b", "a's  b", "a's\n", "a'K", "a'ſt", "'", "''",
    "a'", "a' s", "ア's", M + "'s", "ʰ'll", "a's1", "a's'", "a's's's's", "a'll'll've", "a'l's", "A's'T", "ab's'sx's", "a'sア's", "a's" + M + "'s", "a'd's'm't",
    "a'lſ", "a'Lſ", "a'ſl", "a'vE's", "a'r", "a're", "a'rE.", "a's/", "a's\n/",
    # PUNCT and PTAIL
    "!", "!!", "!" + M + "!", "!!" + M, "!" + M + " ", M + "!", M + "!" + M, "a!", "1!", "! !", "!\t!", "… …", "!\n", "!\n\n", "!\r\n", "!\n/", "!\n//\n", "!/", "!//", "!/\n/", "!\n/\n/x",
    "!\n /", "!\n!", "!\n/!", "!\n" + M, "!\n/" + M, "!\n a", "!\n\na", "! \n", "!\n1", "!/1", "/", "//", "/\n/", "a/b", "a//b", "1/2", "http://x.y/z", "a.\n/b", "😀\n/😀",
    "!'s", "!!'s", "!a's",
    # N
    " 12", "1234567", "a1", "1a", "1A", "12 345", "١٢٣٤٥", "²³", "1²", "x1234567890y", "1.5", "1,234", "1" + M, "1" + M + "a", "1\n", "1/2/3", "12345/\n",
]

ALPHABET = list("ABabsStlLeEvrd'12² \t\n\r/!.…ʰア") + [M, "ſ", "ǅ", "😀", " ", "　"]
# alphabets that lean on one part of the scanner
FOCUS = {
    "case": list("ABCabc") + ["ア", M, "ʰ", "ǅ", " ", "!", "'", "s"],
    "contractions": list("aA'sSlLtTvVeErRdDmM") + ["ſ", "'", "'", " ", "!", "1", "\n"],
    "whitespace": [" ", " ", "\t", "\n", "\n", "\r", " ", "　", "a", "!", "1", "/"],
    "punctuation": list("!./'…") + [M, M, "\n", "\r", " ", "a", "A", "1", "😀"],
}


def random_strings(seed: int, count: int, max_len: int = 24, alphabet=ALPHABET) -> list[str]:
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, max_len))) for _ in range(count)]


# special sets the issue names (none overlaps another or itself; none begins with \s or \p{N})
SPECIAL_SETS = [["<>"], ["<a>", ".x"], ["'s>", "!x"], ["ア."]]
# sets the library refuses, and why
REFUSED_SETS = [(["<a>", "a"], "contains"), (["ab", "<ab>"], "contains"), (["aba"], "suffix"), (["<>", ">x"], "suffix"), (["xy", "yz"], "suffix"), (["<<"], "suffix"),
                ([" x"], "whitespace"), (["\nx"], "whitespace"), (["1x"], "digit"), (["²"], "digit")]
ACCEPTED_SETS = SPECIAL_SETS + [["<|endoftext|>", "<|im_start|>", "<|im_end|>"], ["[PAD]", "[UNK]", "[BOS]", "[EOS]"], ["<>", "<>"]]


def dense(specials, seed: int, count: int, max_len: int = 30) -> list[str]:
    """Random strings in which the specials, their prefixes and the alphabet alternate."""
    rng = random.Random(seed)
    pool = list(specials) * 3 + [t[:-1] for t in specials if len(t) > 1] + ALPHABET
    return ["".join(rng.choice(pool) for _ in range(rng.randint(1, max_len))) for _ in range(count)]


BEHIND_SPECIAL = ["<>…a", "<>😀a", "<>'s", "a<>'s", "a'<>s", "a's<>", "a'll<>", "a'l<>l", "<>.a", "<>\n a", "!<>", "!\n<>", "!\n/<>", " <>", "  <>", "\n <>", "a<>a", "A<>A", "AB<>c",
                  "<><>", "<> a", "<>12345", "12<>345", "1<>", "a <>", "a" + M + "<>", M + "<>", "<>" + M, "<\n >", "<a>.x<a>", ".x.x", "a.x", "a's>", "a's>!x", "'s>'s>", "x's>",
                  "ア.ア.", "Aア.", "ABCア.DE", "!x!x", "!!x", "a!x", "\n!x", "!\n!x"]


def edge_runs() -> list[str]:
    """A run of each chain kind laid against every piece edge around a window edge: it starts k bytes in front of the edge
    and reaches past it; in front of it a letter, an upper-case letter or punctuation."""
    out = []
    for k in range(0, 2 * PIECE + 2):
        for head in (".", "a", "A"):
            for run, tail in (("\n" * 40, " x"), ("\n" + " " * 40, "\nx"), ("\n" + " " * 40, "x"), ("A" * 40, "b"), ("A" * 40, "!"), ("Aア" * 8, "B"), ("Aア" * 8, "Bc"),
                              ("ア" * 14, "A"), ("'s" * 20, "x"), ("!" * 40, "a"), ("\n/" * 20, "a"), (M * 20, "A"), ("  " * 20, "!")):
                fill = "a" * (WIN - k - len(head.encode()))
                out.append(fill + head + run + tail)
    out += ["." + "\n" * (WIN - 1) + " x", "." + "\n" * WIN + " x", "\n" + " " * (WIN - 1) + "\nx", "\n" + " " * (2 * WIN - 1) + "x", "a" + "A" * (WIN - 1) + "b", "a" + "A" * WIN + "!",
            "a" * (WIN - 1) + "'s", "a" * (WIN - 2) + "'ll", "a" * (WIN - 1) + "'ll", "a" * (WIN - 1) + "<>", "!" * (WIN - 1) + "\n/"]
    return out


def long_runs(n_bytes: int = (CARRY + 3) * WIN) -> list[tuple[str, list[int]]]:
    """One run of each chain kind of at least n_bytes bytes (by default more than CARRY windows: the carry kernels take a second
    iteration), with the pre-token offsets worked out by hand (the tests compare them with regex at a small size)."""
    out: list[tuple[str, list[int]]] = []
    k = n_bytes // 3 + 1
    out.append(("x " + "ア" * k + "A", [0, 1, 2 + 3 * k]))                    # all B: the word goes on; the U behind it ends it (UE at the text end)
    k = n_bytes // 4 + 1
    out.append(("Aア" * k + "b!", [0, 4 * k + 1]))                            # U B U B ... l: one word
    out.append(("Aア" * k + "B!", [0, 4 * k, 4 * k + 1]))                     # ... U at the end: the word ends in front of the last U
    out.append(("a" + "A" * n_bytes + "b", [0, 1]))                           # all U, then l: [U]*[l]+
    out.append(("a" + "A" * n_bytes + " ", [0, 1, 1 + n_bytes]))
    out.append((". " + "!" * n_bytes + "\n/a", [0, 1, 2 + n_bytes + 2]))      # all O
    k = n_bytes // 2 + 1
    out.append(("a" + "'s" * k, contraction_chain_offsets(k)))                # 's's's ... alternates: a's | 's's | 's's ...
    out.append(("!" + "\n/" * k + "a", [0, 1 + 2 * k]))                       # \n/ repeated behind punctuation: one token
    out.append(("a" + "\n" * n_bytes + " x", [0, 1, 1 + n_bytes]))            # blank lines
    out.append(("\n" + " " * n_bytes + "x", [0, 1, n_bytes]))
    return out


def contraction_chain_offsets(k: int) -> list[int]:
    """Offsets of "a" + "'s" * k: a's, then 's's as long as two are left, then what remains."""
    out, pos, left = [0], 3, k - 1
    while left >= 2:
        out.append(pos)
        pos += 4
        left -= 2
    if left:
        out.append(pos)
    return out


def chunk_cases() -> list[tuple[str, tuple]]:
    """Chunk starts inside word, punctuation and whitespace runs."""
    return [("ABCdef", (0, 2)), ("ABCdef", (0, 3)), ("ABCアDE", (0, 3)), ("ABCアDE", (0, 6)), ("fooBar", (0, 3)), ("it's", (0, 2)), ("it's", (0, 3)), ("a'll", (0, 3)),
            ("ab's's's", (0, 4)), ("ab's's's", (0, 5)), ("!!" + M + "a", (0, 1)), ("!!" + M + "a", (0, 2)), ("!\n/\n/a", (0, 2)), ("!\n/\n/a", (0, 3)), ("!!!!", (0, 2)),
            (".\n\n\n  x", (0, 2)), (".\n\n\n  x", (0, 1, 4)), ("\n   \n x", (0, 3)), ("\n   \n x", (0, 5)), ("a\n  \n  b", (0, 2, 3, 5)), ("a   b", (0, 2)), ("a   b", (0, 3)),
            ("12345678", (0, 4)), (" a", (0, 1)), ("!a", (0, 1)), ("AB", (0, 1)), ("Ab", (0, 1)), ("A" * (WIN - 2) + "BCd", (0, WIN)), ("\n" + " " * (2 * WIN) + "\nx", (0, WIN + 1)),
            ("a" + "A" * (2 * WIN) + "b", (0, WIN + 1))]


def multilingual(golden_dir, n_bytes: int = 30_000) -> bytes:
    """The head of tests/golden/corpus.en with lines of other scripts, camel case, numbers, contractions in both cases, paths,
    blank lines and indented lines between its lines."""
    rng = random.Random(43)
    lines = (golden_dir / "corpus.en").read_bytes()[:n_bytes].decode("utf-8", errors="ignore").split("\n")
    extra = ["Übergrößenträger … naïve café — «voilà»", "Привет, мир! Это ТЕСТ 2024 года.", "こんにちは世界。１２３４５ ABCアDE", "مرحبا بالعالم ١٢٣٤٥٦",
             "I'M sure THEY'LL say it's fine; we'Ve 12345 of them, don'tknow 'tis", "    indented\n\tand tabbed\r\n\r\n  x", "def fooBar(x):\n    return XMLHttpRequest(x)**2  # ok\n\n\n",
             "😀😀 emoji! 　wide space", "price: $1,234,567.89 on 12/31/1999", "x\n \n \n y", "see https://example.org/a/b/c.html\n//comment\n/path", "e" + M + "cole E" + M + "COLE",
             "HTTPServer fooBar FOObarBAZ ab's's's", "", "", "   "]
    out = []
    for i, line in enumerate(lines):
        out.append(line)
        if i % 3 == 0:
            out.append(rng.choice(extra))
    return "\n".join(out).encode("utf-8")
