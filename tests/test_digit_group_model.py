"""CPU: digit groups (yet-another-bpe_amd/csrc/group_logic.h, the functions the k_grp_* kernels call, run by
tests/hostmodel/group_model.cpp in the kernels' three steps with the kernels' window size) on top of the GPT-2 rules,
against regex.findall with the grouped pattern -- hand-written cases, specials that hold digits, chunk starts inside
digit runs, digit runs against the window edges, random strings.  G = 0 must be the GPT-2 split."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import group_helpers as gh

HM = Path(__file__).resolve().parent / "hostmodel"
GS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libgroup_model.so", HM / "group_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "group_logic.h", csrc / "pretok_logic.h", csrc / "tile_logic.h", csrc / "unicode_classes.inc"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.group_model.restype = ctypes.c_int
    lib.group_special_leads_with_digit.restype = ctypes.c_int
    return lib


def model_split(lib, data: bytes, G: int, specials=(), chunk_starts=(0,)):
    text = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
    n = len(data)
    ch = np.asarray(list(chunk_starts) + [n], dtype=np.uint64)
    sb = [s.encode("utf-8") for s in specials]
    spb = np.frombuffer(b"".join(sb) or b"\0", dtype=np.uint8).copy()
    spo = np.zeros(len(sb) + 1, dtype=np.uint32)
    if sb:
        spo[1:] = np.cumsum([len(x) for x in sb])
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    err = ctypes.c_int64(-1)
    vp = ctypes.c_void_p
    lib.group_model(vp(text.ctypes.data), ctypes.c_uint64(n), vp(ch.ctypes.data), ctypes.c_uint32(len(ch) - 1), vp(spb.ctypes.data),
                    vp(spo.ctypes.data), ctypes.c_uint32(len(sb)), ctypes.c_uint32(G), vp(flags.ctypes.data), ctypes.byref(err))
    assert err.value == -1
    assert set(np.unique(flags[:n]).tolist()) <= {0, 1}  # (no mark of a special's inside is left behind)
    cuts = np.flatnonzero(flags[:n]).tolist() + [n]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def check(lib, s: str, G: int, specials=(), chunk_starts=(0,)):
    data = s.encode("utf-8")
    got, exp = model_split(lib, data, G, specials, chunk_starts), gh.regex_split(data, G, specials, chunk_starts)
    assert got == exp, (s[:80], G, specials, chunk_starts, got[:12], exp[:12])


def test_edge_and_digit_cases(model):
    for G in GS:
        for s in gh.ALL_EDGE:
            check(model, s, G)


def test_group_zero_is_gpt2(model):
    from tests.test_pretok_model import regex_split as gpt2_split

    for s in gh.ALL_EDGE + gh.window_cases()[:2]:
        for sp in ([], ["<x1"], ["<x12", " 12"]):
            assert model_split(model, s.encode("utf-8"), 0, sp) == gpt2_split(s.encode("utf-8"), sp), (s[:80], sp)


def test_specials_that_hold_digits(model):
    for G in GS:
        for sp in gh.SPECIALS:
            assert not any(gh.leads_with_digit(t) for t in sp)
            for s in gh.DIGITS + gh.SPECIAL_TEXTS:
                check(model, s, G, sp)


def test_digit_leading_special_is_recognised(model):
    for tok, lead in [("77", True), ("٣x", True), ("½", True), ("Ⅷ", True), ("<7", False), (" 7", False), ("s1", False), ("x", False), ("é1", False)]:
        b = tok.encode("utf-8")
        assert bool(model.group_special_leads_with_digit(b, ctypes.c_uint32(len(b)))) == lead == gh.leads_with_digit(tok), tok


def test_chunk_start_inside_a_digit_run(model):
    for G in GS:
        for s, cuts in [("1234567890", (0, 4)), ("1234567890", (0, 1, 2, 9)), (" 123456 123456", (0, 3, 10)), ("١٢٣٤٥٦٧", (0, 4, 6)),
                        ("a" * (gh.WIN - 2) + "1234567890", (0, gh.WIN)), ("9" * (2 * gh.WIN + 7), (0, gh.WIN + 1, 2 * gh.WIN))]:
            check(model, s, G, (), cuts)
    rng = random.Random(13)
    for _ in range(400):
        s = "".join(rng.choice("123٣ a<x1") for _ in range(rng.randint(2, 40))).encode("utf-8")
        cuts = sorted({0} | {c for c in (rng.randrange(1, len(s)) for _ in range(rng.randint(0, 3))) if (s[c] & 0xC0) != 0x80})
        G, sp = rng.choice(GS), rng.choice([[], ["<x1"], ["a1", " 12"]])
        assert model_split(model, s, G, sp, cuts) == gh.regex_split(s, G, sp, cuts), (s, G, sp, cuts)


def test_window_cases(model):
    for G in GS:
        for s in gh.window_cases():
            check(model, s, G)
            check(model, s, G, ["<x1"])


def test_random_strings(model):
    rng = random.Random(17)
    for s in gh.random_strings(17, 4000):
        check(model, s, rng.choice(GS), rng.choice(gh.SPECIALS))


def test_large_groups(model):
    for G in (7, 100, 255):
        for s in ["1" * 1000, " " + "9" * 600 + "a" + "8" * 511, "٣" * 700, "1" * (2 * gh.WIN + 3)]:
            check(model, s, G)
