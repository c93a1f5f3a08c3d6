"""CPU: the cl100k split pattern (yet-another-bpe_amd/csrc/split4_logic.h -- the functions k_pt4_fused, k_pt4_special and
the k_nl_* kernels call, run by tests/hostmodel/split4_model.cpp in the kernels' steps with the kernels' piece, window and
carry sizes) against regex.findall with the pattern: one case per rule, special sets dense in the text, chunk starts inside
whitespace runs, runs against every piece and window edge, runs longer than one iteration of the carry, random strings."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import split4_helpers as sh

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libsplit4_model.so", HM / "split4_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src] + [csrc / f for f in ("split4_logic.h", "group_logic.h", "pretok_logic.h", "tile_logic.h", "unicode_classes.inc")]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.split4_model.restype = ctypes.c_int
    lib.split4_special_lead_class.restype = ctypes.c_int
    return lib


def model_flags(lib, data: bytes, G: int, specials=(), chunk_starts=(0,), stage: int = 0) -> np.ndarray:
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
    lib.split4_model(vp(text.ctypes.data), ctypes.c_uint64(n), vp(ch.ctypes.data), ctypes.c_uint32(len(ch) - 1), vp(spb.ctypes.data),
                     vp(spo.ctypes.data), ctypes.c_uint32(len(sb)), ctypes.c_uint32(G), ctypes.c_uint32(stage), vp(flags.ctypes.data),
                     ctypes.byref(err))
    assert err.value == -1
    return flags[:n]


def model_split(lib, data: bytes, G: int, specials=(), chunk_starts=(0,)):
    flags = model_flags(lib, data, G, specials, chunk_starts)
    assert set(np.unique(flags).tolist()) <= {0, 1}  # (no pending position and no mark of a special is left behind)
    cuts = np.flatnonzero(flags).tolist() + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def check(lib, s: str, G: int, specials=(), chunk_starts=(0,)):
    data = s.encode("utf-8")
    got, exp = model_split(lib, data, G, specials, chunk_starts), sh.regex_split(data, G, specials, chunk_starts)
    assert got == exp, (s[:80], s[-40:], G, specials, chunk_starts, got[:12], exp[:12], got[-6:], exp[-6:])


def test_the_oracle_is_the_pattern_of_the_issue():
    assert sh.pattern(3) == (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+")
    assert sh.regex_split("I'LL pay 12345\n\n  now".encode(), 3) == [b"I", b"'LL", b" pay", b" ", b"123", b"45", b"\n\n", b" ", b" now"]


def test_piece_masks_are_the_per_byte_rules(model):
    assert model.split4_masks_selfcheck() == 0


def test_edge_cases(model):
    for G in sh.GS:
        for s in sh.EDGE:
            check(model, s, G)


def test_special_sets_dense_in_the_text(model):
    for i, sp in enumerate(sh.SPECIAL_SETS):
        for G in sh.GS:
            for s in sh.BEHIND_SPECIAL + sh.EDGE:
                check(model, s, G, sp)
                check(model, s.replace("<>", sp[0]), G, sp)
        rng = random.Random(i)
        for s in sh.dense(sp, 100 + i, 1500):
            check(model, s, rng.choice(sh.GS), sp)


def test_pending_is_only_written_behind_a_newline(model):
    """The local pass leaves a position open only where rule 6 says so, and a taken special carries its marks."""
    flags = model_flags(model, ".\n \n  x<>\n y".encode(), 3, ["<>"], stage=1).tolist()
    assert flags == [1, 0, 4, 0, 4, 1, 0, 3, 2, 1, 4, 0]


def test_chunk_starts_inside_whitespace_runs(model):
    for G in sh.GS:
        for s, cuts in sh.chunk_cases():
            check(model, s, G, (), cuts)
    rng = random.Random(29)
    for s in sh.random_strings(29, 1500, 30):
        data = s.encode("utf-8")
        cuts = sorted({0} | {c for c in (rng.randrange(0, len(data)) for _ in range(rng.randint(0, 3))) if (data[c] & 0xC0) != 0x80})
        G, sp = rng.choice(sh.GS), rng.choice([[]] + sh.SPECIAL_SETS)
        assert model_split(model, data, G, sp, cuts) == sh.regex_split(data, G, sp, cuts), (s, G, sp, cuts)


def test_runs_against_piece_and_window_edges(model):
    for s in sh.edge_runs():
        check(model, s, 3)
        check(model, s, 1, ["<>"])


def test_runs_longer_than_one_carry_iteration(model):
    for s in sh.long_runs():
        assert len(s) > sh.CARRY * sh.WIN
        check(model, s, 3)


def test_random_strings(model):
    rng = random.Random(17)
    for s in sh.random_strings(17, 6000):
        check(model, s, rng.choice(sh.GS), rng.choice([[]] + sh.SPECIAL_SETS))


def test_special_lead_class_is_what_the_refusals_look_at(model):
    for tok, cls in [(" x", 2), ("\tx", 2), ("\nx", 2), ("　", 2), ("7x", 1), ("²", 1), ("<7", 3), ("x ", 0), ("é1", 0), ("…", 3)]:
        b = tok.encode("utf-8")
        assert model.split4_special_lead_class(b, ctypes.c_uint32(len(b))) == cls, tok
