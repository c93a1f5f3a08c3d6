"""Shared by the NFC tests (tests/test_nfc_model.py on the CPU model, tests/test_gpu_nfc.py on the device): the strings both
run, and the reference -- unicodedata.normalize("NFC", part) of this interpreter, part by part."""
from __future__ import annotations

import random
import unicodedata as ud

import numpy as np

WIN, PIECE, SHORT, CAP = 4096, 16, 32, 16384   # nfc_logic.h (the model test checks them against the header)
CARRY_TILE = 256 * 8                           # window states per iteration of the carry kernel
# whole-text lengths at which the shared scan code takes another path (tests/group_helpers.py)
TEXT_LENGTHS = (1, 15, 16, 17, WIN - 1, WIN, WIN + 1, CARRY_TILE * WIN, CARRY_TILE * WIN + 1)


def nfc(s: str) -> str:
    return ud.normalize("NFC", s)


def code_points():
    return [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]


def quick_check_sets():
    """(Maybe, No) code points, derived as tools/gen_unicode_norm.py derives them."""
    seconds = set()
    for cp in code_points():
        d = ud.decomposition(chr(cp))
        if d and not d.startswith("<"):
            parts = [int(x, 16) for x in d.split()]
            if len(parts) == 2 and not 0xAC00 <= cp < 0xAC00 + 11172 and nfc(chr(parts[0]) + chr(parts[1])) == chr(cp):
                seconds.add(parts[1])
    maybe = sorted(seconds | set(range(0x1161, 0x1176)) | set(range(0x11A8, 0x11C3)))
    no = [cp for cp in code_points() if nfc(chr(cp)) != chr(cp)]
    return maybe, no


_ALPHABET = None


def alphabet():
    """All Maybe code points, 400 No code points, U+0300..036F, Hangul L / V / T / LV / LVT, the non-starter decompositions
    U+0F73 / U+0344, the Indic and Balinese two-part vowels, a few plain starters."""
    global _ALPHABET
    if _ALPHABET is None:
        maybe, no = quick_check_sets()
        rng = random.Random(5)
        a = list(maybe) + rng.sample(no, 400) + list(range(0x300, 0x370))
        a += [0x1100, 0x1105, 0x1112, 0x1161, 0x1169, 0x1175, 0x11A8, 0x11AF, 0x11C2, 0xAC00, 0xAC1C, 0xD788, 0xAC01, 0xB000, 0xD7A3]
        a += [0x0F73, 0x0344, 0x0F71, 0x0F72, 0x0F74, 0x0F75, 0x0F81]
        a += [0x09C7, 0x09BE, 0x09D7, 0x09CB, 0x09CC, 0x0B47, 0x0B56, 0x0B3E, 0x0B57, 0x0B4B, 0x0BC6, 0x0BC7, 0x0BBE, 0x0BD7, 0x0BCA, 0x0BCC,
              0x0CC6, 0x0CC2, 0x0CD5, 0x0CD6, 0x0CCA, 0x0CCB, 0x0D46, 0x0D47, 0x0D3E, 0x0D57, 0x0D4A, 0x0DD9, 0x0DCA, 0x0DCF, 0x0DDF, 0x0DDC, 0x0DDD,
              0x1B05, 0x1B35, 0x1B06, 0x1B3A, 0x1B3C, 0x1B3B, 0x1B3E, 0x1B40, 0x1B42, 0x1B43, 0x1025, 0x102E, 0x1026]
        a += [ord(c) for c in "aeAo .1"] + [0xE9, 0x4E2D, 0x1F600, 0x0591, 0x05B0, 0x0E01]
        _ALPHABET = a
    return _ALPHABET


def random_strings(seed: int, count: int, max_len: int = 12):
    rng = random.Random(seed)
    a = alphabet()
    marks = list(range(0x300, 0x370))
    out = []
    for _ in range(count):
        k = rng.randint(1, max_len)
        r = rng.random()
        pool = marks + [0x61, 0x1100, 0x1161, 0x11A8] if r < 0.2 else a
        out.append("".join(chr(rng.choice(pool)) for _ in range(k)))
    return out


def assert_kinds(strings) -> None:
    """The list holds strings that grow, shrink, stay, are only reordered, and compose across two starters."""
    grow = shrink = stay = reorder = two = False
    for s in strings:
        t = nfc(s)
        a, b = len(s.encode()), len(t.encode())
        grow |= b > a
        shrink |= b < a
        stay |= s == t
        reorder |= s != t and sorted(s) == sorted(t)
        two |= any(ud.combining(x) == 0 and ud.combining(y) == 0 and len(nfc(x + y)) == 1 for x, y in zip(s, s[1:]))
    assert grow and shrink and stay and reorder and two, (grow, shrink, stay, reorder, two)


DIRTY = ["e\u0301", "a\u0323\u0301", "a\u0301\u0323", "\u1100\u1161\u11a8", "\uac00\u11a8", "\u0958", "\u0344", "\u0f73\u0f71", "\u09c7\u09be",
         "\u212b", "\U0001d1c0", "\u1e0b\u0323", "q\u0307\u0323", "\u0340\u0341", "\u2126x\u0301"]


def edge_cases():
    """Dirty segments at every position around a window edge."""
    out = []
    for edge in (WIN, 2 * WIN):
        for seg in ("e\u0301", "a\u0323\u0301\u0300", "\u1100\u1161\u11a8"):
            nb = len(seg.encode())
            for pos in range(edge - nb - 1, edge + 2):
                out.append("x" * pos + seg + "yz")
    return out


def carry_cases():
    """... and around the edge of the carry kernel's tile of windows (8 MiB each): a train of 4-byte dirty segments across the
    edge, in the four phases, so that every position of a segment against the edge occurs."""
    edge = CARRY_TILE * WIN
    return ["x" * (edge - 22 - phase) + "e\u0301y" * 12 + "z" for phase in range(4)]


def length_cases():
    """Segments of 31, 32 and 33 decomposed code points (reordered marks, and a decomposing base), long non-starter runs for the
    counting sort, and many short runs inside one long segment."""
    out = []
    for n in (SHORT - 1, SHORT, SHORT + 1, 100, 1000):
        out.append("a" + "\u0301\u0323" * ((n - 1) // 2) + "\u0300" * ((n - 1) % 2))
        out.append("\u00e9" + "\u0323" * (n - 2))            # e + U+0301, then ccc 220 marks: reordered in front of the accent
        out.append("\u1100" + "\u1161\u11a8\u1100" * (n // 3) + "\u1161" * (n % 3))  # L starts a segment each time
        out.append("\u0958" * n)                             # quick-check No starters: n runs of one mark
        rng = random.Random(n)
        out.append("o" + "".join(chr(rng.choice((0x301, 0x323, 0x327, 0x31b, 0x345, 0x308))) for _ in range(n - 1)))
    return out


def part_cases():
    """(text bytes, part starts): parts that begin with a mark, empty parts, a part cut inside a dirty segment."""
    out = []
    t = "e\u0301a\u0323\u0301".encode()
    out.append((t, [0, 1]))            # cut between e and its accent: the accent starts a part and stays
    out.append((t, [0, 3, 4]))         # cut inside a\u0323\u0301
    out.append((t, [0, 0, 3, 3, len(t), len(t)]))
    out.append(("\u0301\u0301abc\u0323\u0301".encode(), [0, 2]))
    out.append(("\u1100\u1161\u11a8".encode(), [0, 3, 6]))   # jamo in parts of their own: nothing composes
    out.append((b"", [0]))
    out.append((b"", [0, 0, 0]))
    out.append(("x\u0344".encode(), [0, 1]))
    return out


def pack(strings):
    """strings (str or bytes) as one buffer of parts -> (u8 array, u64 part starts)"""
    bs = [s.encode("utf-8") if isinstance(s, str) else s for s in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy(), off[:-1].copy()


def reference(data: bytes, starts):
    """-> (normalised bytes, n_parts + 1 offsets): every part on its own through unicodedata"""
    cuts = [int(x) for x in starts] + [len(data)]
    parts = [nfc(data[a:b].decode("utf-8")).encode("utf-8") for a, b in zip(cuts[:-1], cuts[1:])]
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return b"".join(parts), off


def training_text(golden_dir, n_bytes: int = 12_000) -> bytes:
    """The multilingual text of the split tests with Korean lines, in NFD, followed by its NFC: without a normaliser the two
    halves are different byte strings, with one they are the same words twice."""
    from tests import split5_helpers as sh

    text = sh.multilingual(golden_dir, n_bytes).decode("utf-8") + "\n" + "\ud55c\uad6d\uc5b4 \ud14d\uc2a4\ud2b8 \uc815\uaddc\ud654 \uc2dc\ud5d8 \uac00\uac01\uac04 \u00e9t\u00e9 na\u00efve\n" * 20
    return (ud.normalize("NFD", text) + "\n" + ud.normalize("NFC", text)).encode("utf-8")


def normalized_words(data: bytes, starts, split):
    """The words a trainer with normalizer="nfc" must see: every chunk normalised on its own by unicodedata, then
    split(normalised bytes, chunk starts in them) -- regex's words of the normalised chunks."""
    norm, off = reference(data, starts)
    return split(norm, off[:-1])


ENCODE_TEXTS = ["plain ASCII text, nothing to do", "caf\u00e9 d\u00e9j\u00e0 vu", "cafe\u0301 de\u0301ja\u0300 vu", "\u1112\u1161\u11ab\u1100\u116e\u11a8\u110b\u1165 and \ud55c\uad6d\uc5b4",
                "<|e|>\u0338 is no special, <|e|> is", "a<|e|>e\u0301<a>\u0323x", "q\u0307\u0323 \u0958 \u212b \u2126 12345", "", "\u0301starts with a mark",
                "x" + "\u0323\u0301" * 40 + "y", "\u00e9" * 300 + "e\u0301" * 300, "\uac00\u11a8 \u1100\u1161\u11a8 \u09c7\u09be \U0001d1c0"]
