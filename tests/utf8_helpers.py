"""Shared by the tests of errors="replace" / "ignore" (tests/test_utf8_model.py on the CPU model, tests/test_utf8_api.py on the
host route, tests/test_gpu_utf8.py on the device): the byte strings all of them run, the damaged corpus, and the reference --
bytes.decode("utf-8", errors=mode).encode() of this interpreter, part by part."""
from __future__ import annotations

import codecs
import itertools
import random

import numpy as np

from tests import decode_helpers

MODES = {"replace": 1, "ignore": 2}   # include/yabpe.h: YABPE_UTF8_REPLACE, YABPE_UTF8_IGNORE
PIECE, TILE = 16, 4096                # utf8_logic.h (the model test checks them against the header)
HIGH = [b for b in decode_helpers.CLASS_BYTES if b >= 0x80]


def repair(part: bytes, mode: str) -> bytes:
    return part.decode("utf-8", errors=mode).encode("utf-8")


def ill_formed(part: bytes) -> bool:
    try:
        part.decode("utf-8")
    except UnicodeDecodeError:
        return True
    return False


_seen: list[int] = []


def _record(e):
    _seen.append(e.start)
    return "�", e.end


codecs.register_error("tests_utf8_record", _record)


def subparts(part: bytes) -> list[int]:
    """The starts of the ranges CPython's error handler is called for: one per maximal subpart."""
    del _seen[:]
    part.decode("utf-8", errors="tests_utf8_record")
    return list(_seen)


def reference(data: bytes, starts, mode: str):
    """-> (repaired bytes, n_parts + 1 offsets, subparts, position of the first ill-formed byte or -1): part by part"""
    cuts = [int(x) for x in starts] + [len(data)]
    out, off, n_sub, first = [], [0], 0, -1
    for a, b in zip(cuts[:-1], cuts[1:]):
        out.append(repair(data[a:b], mode))
        off.append(off[-1] + len(out[-1]))
        if len(out[-1]) != b - a or out[-1] != data[a:b]:
            bad = subparts(data[a:b])
            n_sub += len(bad)
            if first < 0 and bad:
                first = a + bad[0]
    return b"".join(out), off, n_sub, first


def pack(parts):
    """byte strings as one buffer of parts -> (u8 array, u64 part starts)"""
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(b) for b in parts])
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off[:-1].copy()


# ---------------------------------------------------------------- the lists
def short_strings() -> list[bytes]:
    """Every byte string of length 1 to 4 over one byte of each UTF-8 class."""
    return [bytes(s) for n in range(1, 5) for s in itertools.product(decode_helpers.CLASS_BYTES, repeat=n)]


def random_strings(count: int = 100_000) -> list[bytes]:
    rng = random.Random(11)
    return [decode_helpers.random_bytes(rng, rng.randint(5, 60)) for _ in range(count)]


def ill_formed_sequences() -> list[bytes]:
    """Every ill-formed string of 1 to 3 class bytes that neither begins nor ends with ASCII (an ASCII byte at either end only
    moves the sequence): every lead with every way of not completing it, every stray byte, alone and in twos and threes."""
    return [bytes(s) for n in range(1, 4) for s in itertools.product(decode_helpers.CLASS_BYTES, repeat=n)
            if s[0] >= 0x80 and s[-1] >= 0x80 and ill_formed(bytes(s))]


def edge_cases(edge: int, seqs) -> list[bytes]:
    """Parts for one call: a filler of edge / 2 bytes, then parts of `edge` bytes with a sequence at offsets -3 .. +3 around their
    middle, between letters -- in the packed text that is around a multiple of `edge`."""
    out = [b"x" * (edge // 2)]
    for s in seqs:
        for d in range(-3, 4):
            t = b"x" * (edge // 2 + d) + s
            out.append(t + b"y" * (edge - len(t)))
    return out


def cut_cases() -> list[tuple[bytes, list[int]]]:
    """(text, part starts): part cuts at every position inside E2 82 AC and F0 9F 98 80, alone and between letters, one cut and
    all pairs of cuts; empty parts around them."""
    out = []
    for ch in (b"\xe2\x82\xac", b"\xf0\x9f\x98\x80"):
        for pre, post in ((b"", b""), (b"ab", b"cd"), (ch, ch)):
            t, a = pre + ch + post, len(pre)
            for i in range(0, len(ch) + 1):
                out.append((t, sorted({0, a + i})))
                out.append((t, [0, 0] + [a + i, a + i]))
                for j in range(i, len(ch) + 1):
                    out.append((t, sorted({0, a + i, a + j})))
    return out


# ---------------------------------------------------------------- the damaged corpus
DAMAGE_RATE = 500          # one byte in this many becomes a class byte >= 0x80
CHUNK = 1 << 12            # chunk_size_bytes of the trainers that read it


def damaged_corpus(golden_dir, extra: bytes = b"") -> bytes:
    """tests/golden/corpus.en (+ extra) with a seeded 1 in DAMAGE_RATE bytes replaced by a class byte >= 0x80, and a truncated
    lead (E2 82, F0 9F 98 or C3) right in front of every fifth chunk cut of a trainer with chunk_size_bytes = CHUNK: the cuts
    are walked as chunk_ranges makes them (CHUNK bytes on, back over at most 4 continuation bytes), and a space behind the
    truncated lead keeps that cut where it is.  One cut falls inside E2 82 82 82 82 82 82: read as one text that is U+2082 and
    four stray bytes, read as two chunks a truncated lead and five."""
    data = bytearray((golden_dir / "corpus.en").read_bytes() + extra)
    rng = random.Random(13)
    for _ in range(len(data) // DAMAGE_RATE):
        data[rng.randrange(len(data))] = rng.choice(HIGH)
    leads = itertools.cycle((b"\xe2\x82", b"\xf0\x9f\x98", b"\xc3"))
    start, k = 0, 0
    while start + CHUNK < len(data):
        stop = start + CHUNK
        if k % 5 == 3:
            lead = next(leads)
            data[stop - len(lead):stop] = lead
            data[stop] = 0x20
        elif k == 1:  # more continuation bytes than a cut steps back over: the cut falls between them, behind E2 82
            data[stop - 6:stop + 2] = b"\xe2" + b"\x82" * 6 + b" "
            stop -= 4
        else:
            while stop > start + CHUNK - 4 and data[stop] & 0xC0 == 0x80:
                stop -= 1
        start, k = stop, k + 1
    return bytes(data)


def chunk_words(data: bytes, starts, mode: str, split, nfc: bool = False) -> list[bytes]:
    """The words a trainer with errors=mode must see: every chunk repaired on its own by bytes.decode (then normalised by
    unicodedata), then split(those bytes, the chunk starts in them) -- regex's words of chunk.decode(errors=mode)."""
    from tests import nfc_helpers

    fixed, off, _n, _first = reference(data, starts, mode)
    if nfc:
        return nfc_helpers.normalized_words(fixed, off[:-1], split)
    return split(fixed, off[:-1])
