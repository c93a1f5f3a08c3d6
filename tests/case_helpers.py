"""Shared by the lower-casing tests (tests/test_case_model.py on the CPU model, tests/test_gpu_case.py on the device): the
strings both run, and the reference -- str.lower() of this interpreter, part by part."""
from __future__ import annotations

import random

import numpy as np

WIN, PIECE = 4096, 16                 # case_logic.h (the model test checks them against the header)
CARRY_TILE = 256 * 8                  # window states per iteration of the carry kernel
TEXT_LENGTHS = (1, 15, 16, 17, WIN - 1, WIN, WIN + 1, CARRY_TILE * WIN, CARRY_TILE * WIN + 1)
SIGMA, FINAL, SMALL = "\u03a3", "\u03c2", "\u03c3"
KELVIN, DOTTED_I, A_STROKE = "\u212a", "\u0130", "\u023a"   # 3 -> 1 byte, 2 -> 3 bytes (two code points), 2 -> 3 bytes


def code_points():
    return [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]


_CLASSES = None


def classes():
    """(changing, cased for the rule, ignorable) code points, derived from str.lower() as tools/gen_unicode_case.py derives them."""
    global _CLASSES
    if _CLASSES is None:
        changing, cased, ign = [], [], []
        for cp in code_points():
            c = chr(cp)
            if c.lower() != c:
                changing.append(cp)
            if ("a" + SIGMA + c).lower()[1] == SMALL:
                cased.append(cp)
            elif ("a" + SIGMA + c + "a").lower()[1] == SMALL:
                ign.append(cp)
        _CLASSES = (changing, cased, ign)
    return _CLASSES


def resized():
    return [cp for cp in classes()[0] if len(chr(cp).lower().encode()) != len(chr(cp).encode())]


_ALPHABET = None


def alphabet():
    """Covers every class: the sigmas, the length changers, cased letters that change and that do not, ignorables of 1 to 4
    bytes, code points that are neither, in every UTF-8 length."""
    global _ALPHABET
    if _ALPHABET is None:
        changing, cased, ign = classes()
        rng = random.Random(7)
        a = [0x3A3, 0x3C3, 0x3C2] + resized()
        a += [ord(c) for c in "aZq'.:^` 1-\n"]
        a += [0xC9, 0xE9, 0x410, 0x44F, 0x391, 0x3B1, 0x1E9E, 0x10400, 0x10428, 0x1D400, 0x2160, 0x24B6]   # cased, 2 to 4 bytes
        a += [0xAD, 0x300, 0x307, 0x2019, 0x200B, 0xFE00, 0x1F3FB, 0xE0001, 0xE0100, 0x5B0]                 # ignorable, 2 to 4 bytes
        a += [0x4E2D, 0xAC00, 0x1F600, 0x5D0, 0x660, 0x2014]                                                # neither
        a += rng.sample(changing, 60) + rng.sample(cased, 40) + rng.sample(ign, 40)
        _ALPHABET = a
    return _ALPHABET


def class_alphabet():
    """One short list that still holds every class in every UTF-8 length: for x + sigma + y over all pairs."""
    return ["", "a", "Z", "'", ".", " ", "1", "\u00e9", "\u0410", "\u00ad", "\u0301", "\u2019", "\u4e2d", "\u1e9e", "\ufe00", "\U00010400", "\U0001f600",
            "\U000e0001", SIGMA, SMALL, FINAL, KELVIN, DOTTED_I, A_STROKE, "'\u0301\u00ad", "a'", "'a", " '", "' "]


def random_strings(seed: int, count: int, max_len: int = 12):
    rng = random.Random(seed)
    a = alphabet()
    sig = [0x3A3, 0x3A3, 0x27, 0x2E, 0x61, 0x41, 0x20, 0x301, 0xAD, 0x391]
    out = []
    for _ in range(count):
        k = rng.randint(1, max_len)
        pool = sig if rng.random() < 0.35 else a
        out.append("".join(chr(rng.choice(pool)) for _ in range(k)))
    return out


SIGMAS = ["\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3",        # final at the end, not final inside
          "\u03a3", "a\u03a3", "\u03a3a", "a\u03a3a", "A\u03a3 B", "a\u03a3.", "a.\u03a3", "a\u03a3.a", "a'\u03a3'", "a'\u03a3'b", " '\u03a3", "a\u0301\u03a3\u0301",
          "a\u03a3\u00ad\u0301'\u03b1", "\u03a3\u03a3", "a\u03a3\u03a3", "\u03a3\u03a3\u03a3 \u03a3", "1\u03a3", "a1\u03a3", "\u4e2d\u03a3", "\U00010400\u03a3\U0001f600"]
GROW = [DOTTED_I, A_STROKE, "\u023e", "x" + DOTTED_I * 9 + "y", A_STROKE * 20]
SHRINK = [KELVIN, "\u2126", "\u212b", "\u1e9e", "\u2c62\u2c64\u2c6d", KELVIN * 33 + "z"]
SAME_SIZE = ["", "plain lower case", "caf\u00e9 \u4e2d\u6587 \ud55c\uad6d\uc5b4 \U0001f600", "Hello, World", "\u041f\u0420\u0418\u0412\u0415\u0422 \u039a\u0391\u039b\u0397", "\u00c0\u00c9\u00ce\u00d5\u00dc"]


def assert_kinds(strings, part_lists=()) -> None:
    """The lists hold strings that grow, shrink and stay, and a sigma in each position: final, not final, final only because
    of a part end, and separated by ignorables on either side (one that stays final, one that does not)."""
    _changing, cased, ign = classes()
    cased, ign = set(cased), set(ign)
    grow = shrink = stay = final = nonfinal = ign_front = ign_behind = False
    for s in strings:
        t = s.lower()
        a, b = len(s.encode()), len(t.encode())
        grow |= b > a
        shrink |= b < a
        stay |= s == t
        for i, ch in enumerate(s):
            if ch != SIGMA:
                continue
            # (one lowered code point per code point up to i unless a dotted I came before: skip those strings)
            if DOTTED_I in s[:i]:
                continue
            final |= t[i] == FINAL
            nonfinal |= t[i] == SMALL
            ign_front |= i > 1 and ord(s[i - 1]) in ign and t[i] == FINAL
            ign_behind |= i + 2 < len(s) and ord(s[i + 1]) in ign and ord(s[i + 2]) in cased and t[i] == SMALL
    part_end = False
    for data, starts in part_lists:
        whole = data.decode("utf-8").lower().encode("utf-8")
        part_end |= FINAL.encode() in reference(data, starts)[0] and FINAL.encode() not in whole
    assert grow and shrink and stay and final and nonfinal and ign_front and ign_behind, (grow, shrink, stay, final, nonfinal, ign_front, ign_behind)
    assert part_end or not part_lists


def edge_cases():
    """Length changers and sigmas at every position around a piece edge and a window edge."""
    out = []
    for edge in (PIECE, 2 * PIECE, WIN, 2 * WIN):
        for seg in (KELVIN, DOTTED_I, "a" + SIGMA, "a" + SIGMA + "'a", "\U00010400", "a'" + SIGMA + "'\u0301"):
            nb = len(seg.encode())
            for pos in range(edge - nb - 1, edge + 2):
                out.append("x" * pos + seg + "yz")
                out.append("\u0416" * (pos // 2) + "x" * (pos % 2) + seg)
    return out


def carry_cases():
    """... and around the edge of the carry kernel's tile of windows (8 MiB each): a sigma whose cased neighbour lies across
    the edge behind a run of ignorables, from either side, and a train of length changers over it."""
    edge = CARRY_TILE * WIN
    return ["x" * (edge - 9) + "a" + SIGMA + "'" * 12 + "b",          # the sigma in front of the edge, its cased follower behind it
            "x" * (edge - 9) + "a" + SIGMA + "'" * 12 + " b",         # ... a space instead: final
            "x" * (edge - 8) + "a" + "'" * 12 + SIGMA + " ",          # the sigma behind the edge, its cased predecessor in front
            "x" * (edge - 8) + " " + "'" * 12 + SIGMA + " ",
            "x" * (edge - 20) + (KELVIN + DOTTED_I) * 8 + "z"]


def length_cases():
    """Whole-text lengths (in bytes) with a length-changing code point and a sigma at the last byte and at the first."""
    out = ["A", "'"]  # (one byte holds neither: a capital and an ignorable)
    for n in TEXT_LENGTHS:
        for tail in (KELVIN, DOTTED_I, "a" + SIGMA, SIGMA):
            nb = len(tail.encode())
            if n >= nb:
                out.append("x" * (n - nb) + tail)
                out.append(tail + "x" * (n - nb))
    return out


def part_cases():
    """(text bytes, part starts): a sigma that is final only because its part ends, one that is not final only inside its
    part, empty parts, parts that start with an ignorable."""
    out = []
    t = ("a" + SIGMA + "b" + SIGMA + "'c").encode()
    out.append((t, [0, 3]))                 # a + sigma | b + sigma + ' + c
    out.append((t, [0, 1, 3, 4, 6]))        # sigma after a part start: no cased code point in front
    out.append((t, [0, 0, 3, 3, len(t), len(t)]))
    out.append((t, [0, 6]))                 # b + sigma | ' + c: final by the part end
    out.append(((KELVIN + DOTTED_I + "x").encode(), [0, 3, 5]))
    out.append((b"", [0]))
    out.append((b"", [0, 0, 0]))
    out.append((("A" * 40 + SIGMA).encode() + ("'" * 40 + "a").encode(), [0, 42]))
    return out


def ignorable_runs(n: int = 1 << 20):
    """sigma + n apostrophes + a cased letter, and a cased letter + n apostrophes + sigma: linear, whatever the run."""
    return ["a" + SIGMA + "'" * n + "b", "a" + SIGMA + "'" * n + " ", "a" + "'" * n + SIGMA, " " + "'" * n + SIGMA]


def pack(strings):
    """strings (str or bytes) as one buffer of parts -> (u8 array, u64 part starts)"""
    bs = [s.encode("utf-8") if isinstance(s, str) else s for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy(), off[:-1].copy()


def reference(data: bytes, starts):
    """-> (lowered bytes, n_parts + 1 offsets): every part on its own through str.lower()"""
    cuts = [int(x) for x in starts] + [len(data)]
    parts = [data[a:b].decode("utf-8").lower().encode("utf-8") for a, b in zip(cuts[:-1], cuts[1:])]
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return b"".join(parts), off


def model_strings():
    """The strings of the model test that the device test runs as parts of one buffer."""
    return SIGMAS + GROW + SHRINK + SAME_SIZE + random_strings(11, 3000) + edge_cases()


def training_text(golden_dir, n_bytes: int = 12_000) -> bytes:
    """The NFC tests' training text with the first letter of every word capitalised and a Greek line in capitals: with
    lowercase the capitalised words are the plain ones again, without it they are other words."""
    from tests import nfc_helpers as nh

    text = nh.training_text(golden_dir, n_bytes).decode("utf-8")
    words = text.split(" ")
    text = " ".join(w[:1].upper() + w[1:] if i % 2 else w for i, w in enumerate(words))
    greek = "\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 \u039a\u0391\u0399 \u039f\u0399 \u03a3\u03a5\u039d\u03a4\u03a1\u039f\u03a6\u039f\u0399 \u03a4\u039f\u03a5\u03a3 \u0130stanbul \u212aelvin\n" * 20
    return (text + "\n" + greek).encode("utf-8")


def lowered_words(data: bytes, starts, split, nfc: bool = False):
    """The words a trainer with lowercase=True must see: every chunk lowered (then normalised) on its own, then
    split(bytes, chunk starts in them) -- regex's words of the lowered chunks."""
    import unicodedata as ud

    cuts = [int(x) for x in starts] + [len(data)]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = data[a:b].decode("utf-8").lower()
        parts.append((ud.normalize("NFC", s) if nfc else s).encode("utf-8"))
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return split(b"".join(parts), off[:-1])


ENCODE_TEXTS = ["plain ascii text, nothing to do", "Hello, World! It's 42", "CAF\u00c9 D\u00c9J\u00c0 VU", "\u041f\u0420\u0418\u0412\u0415\u0422 \u041c\u0418\u0420",
                "\u039f\u0394\u03a5\u03a3\u03a3\u0395\u03a5\u03a3 \u039a\u0391\u0399 \u03a3", "\u0130STANBUL \u212aELVIN \u023a", "<|E|> is no special, <|e|> is", "A<|e|>B<a>C", "",
                "\u03a3", "a\u03a3'''", "I\u0307\u0323 \u0130\u0316", "X" * 300 + "\u03a3" * 3 + "\u0130" * 100, "\ud55c\uad6d\uc5b4 \u4e2d\u6587 \U0001f600 MiXeD"]
