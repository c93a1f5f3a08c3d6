"""CPU: the rules of lower-casing (yet-another-bpe_amd/csrc/case_logic.h, the functions the HIP kernels call) and the tables of
csrc/unicode_case.inc against str.lower() of this interpreter -- every code point, the facts the design rests on, x + sigma + y
over a class-covering alphabet, random strings, pieces and windows around 16, 4096 and the carry tile, and parts."""
from __future__ import annotations

import ctypes
import subprocess
import unicodedata
from pathlib import Path

import numpy as np
import pytest

from tests import case_helpers as ch

HM = Path(__file__).resolve().parent / "hostmodel"
CP, CASED, IGN, TWO = 0x1FFFFF, 1 << 21, 1 << 22, 1 << 23


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libcase_model.so", HM / "case_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "case_logic.h", csrc / "unicode_case.inc", csrc / "pretok_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.case_model.restype = ctypes.c_int
    lib.case_model_version.restype = ctypes.c_char_p
    lib.case_model_ascii_state.restype = ctypes.c_uint32
    lib.case_model_upper_bits4.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def table(model):
    tab = np.zeros(0x110000, np.uint32)
    model.case_model_table(ctypes.c_void_p(tab.ctypes.data))
    return tab


def run_model(lib, data, starts):
    """-> (rc, bytes, offsets list, counts list)"""
    data, starts = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(starts, np.uint64)
    cap = len(data) + len(data) // 2 + 16
    out, off = np.zeros(cap, np.uint8), np.zeros(len(starts) + 1, np.uint64)
    n, counts = ctypes.c_uint64(0), np.zeros(6, np.uint64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.case_model(vp(data), ctypes.c_uint64(len(data)), vp(starts), ctypes.c_uint32(len(starts)), vp(out), ctypes.c_uint64(cap),
                        ctypes.byref(n), vp(off), vp(counts))
    return rc, out[:n.value].tobytes(), off.tolist(), counts.tolist()


def check_parts(lib, parts):
    data, starts = ch.pack(parts)
    rc, got, off, counts = run_model(lib, data, starts)
    assert rc == 0, rc
    exp, exp_off = ch.reference(data.tobytes(), starts)
    assert off == exp_off
    assert got == exp
    return counts


def test_version(model):
    have = model.case_model_version().decode()
    assert have == unicodedata.unidata_version, (
        f"csrc/unicode_case.inc was generated for Unicode {have}, this interpreter has {unicodedata.unidata_version}: "
        "rerun the generator (python tools/gen_unicode_case.py)")
    sizes = np.zeros(2, np.uint32)
    model.case_model_sizes(ctypes.c_void_p(sizes.ctypes.data))
    assert sizes.tolist() == [ch.PIECE, ch.WIN]


def test_tables_for_every_code_point(table):
    changing, cased, ign = ch.classes()
    low = (table & CP).tolist()
    two = np.flatnonzero(table & TWO).tolist()
    assert two == [0x130]
    for cp in ch.code_points():
        exp = chr(cp).lower()
        got = chr(low[cp]) + ("\u0307" if cp == 0x130 else "")
        assert got == exp, hex(cp)
    assert np.flatnonzero(table & CASED).tolist() == cased
    assert np.flatnonzero(table & IGN).tolist() == ign
    assert not np.any((table & CASED != 0) & (table & IGN != 0))
    assert all(low[cp] == cp for cp in range(0xD800, 0xE000))


def test_facts_the_design_rests_on(model, table):
    changing, cased, ign = ch.classes()
    assert len(changing) == 1393 and min(cp for cp in changing if cp > 0x7F) == 0xC0
    assert [cp for cp in changing if len(chr(cp).lower()) != 1] == [0x130] and chr(0x130).lower() == "i\u0307"
    resized = ch.resized()
    assert len(resized) == 25
    grow = [cp for cp in resized if len(chr(cp).lower().encode()) > len(chr(cp).encode())]
    assert grow == [0x130, 0x23A, 0x23E] and all(len(chr(cp).encode()) == 2 and len(chr(cp).lower().encode()) == 3 for cp in grow)
    assert len("\u212a".encode()) == 3 and "\u212a".lower() == "k"
    assert min(len(chr(cp).lower().encode()) / len(chr(cp).encode()) for cp in resized) == 1 / 3
    assert all(2 * len(chr(cp).lower().encode()) <= 3 * len(chr(cp).encode()) for cp in ch.code_points())   # at most 1.5 x
    assert all(chr(cp).lower().lower() == chr(cp).lower() for cp in changing)                               # idempotent
    assert len(cased) == 4141 and len(ign) == 2413
    assert [chr(cp) for cp in ign if cp < 0x80] == ["'", ".", ":", "^", "`"]
    # the same classes from the front
    assert all((chr(cp) + ch.SIGMA).lower()[-1] == ch.FINAL for cp in cased[::7])
    assert all(("a" + chr(cp) + ch.SIGMA).lower()[-1] == ch.FINAL for cp in ign[::5])
    # both sigmas and the capital are two bytes; the capital is cased and changes
    assert {len(c.encode()) for c in (ch.SIGMA, ch.FINAL, ch.SMALL)} == {2}
    assert table[0x3A3] & CP == 0x3C3 and table[0x3A3] & CASED
    # the ASCII shortcuts of the kernels against the table
    for b in range(128):
        st = 1 if table[b] & CASED else 0 if table[b] & IGN else 2
        assert model.case_model_ascii_state(ctypes.c_uint32(b)) == st, b
        w = b | b << 8 | b << 16 | b << 24
        assert model.case_model_upper_bits4(ctypes.c_uint32(w)) == (0x20202020 if 65 <= b <= 90 else 0), b
    assert model.case_model_upper_bits4(ctypes.c_uint32(0x5B5A4140)) == 0x00202000


def test_kinds():
    ch.assert_kinds(ch.SIGMAS + ch.GROW + ch.SHRINK + ch.SAME_SIZE, ch.part_cases())


def test_named_strings(model):
    counts = check_parts(model, ch.SIGMAS + ch.GROW + ch.SHRINK + ch.SAME_SIZE)
    assert counts[5] == 2 and counts[3] > 0 and 0 < counts[4] < counts[3]
    for s in ch.SIGMAS + ch.GROW + ch.SHRINK + ch.SAME_SIZE:
        check_parts(model, [s])
    assert check_parts(model, ["plain lower case"])[5] == 0
    assert check_parts(model, ["Hello, World \u00c9\u0416"])[1:6] == [4, 0, 0, 0, 1]
    assert check_parts(model, [ch.KELVIN])[1:6] == [1, 1, 0, 0, 2]
    assert check_parts(model, ["a" + ch.SIGMA])[1:6] == [1, 0, 1, 1, 2]


def test_every_changing_code_point(model):
    changing = ch.classes()[0]
    check_parts(model, [chr(cp) for cp in changing])
    check_parts(model, ["".join(chr(cp) for cp in changing)])
    check_parts(model, ["x" + chr(cp) + "\u0416" for cp in changing])


def test_sigma_between_every_pair(model):
    a = ch.class_alphabet()
    parts = [x + ch.SIGMA + y for x in a for y in a]
    check_parts(model, parts)
    for s in parts[::13]:
        check_parts(model, [s])
    check_parts(model, ["".join(parts)])


def test_random_strings(model):
    parts = ch.random_strings(3, 200_000)
    assert len(parts) == 200_000
    check_parts(model, parts)
    check_parts(model, ["".join(parts[:20_000])])  # ... and as one text


def test_pieces_and_windows(model):
    parts = ch.edge_cases()
    check_parts(model, parts)
    for s in parts[::3]:
        check_parts(model, [s])


def test_whole_text_lengths(model):
    for s in ch.length_cases():
        assert len(s.encode()) in ch.TEXT_LENGTHS
        if len(s) <= 2 * ch.WIN:
            check_parts(model, [s])
    big = [s for s in ch.length_cases() if len(s) > 2 * ch.WIN]
    for s in big[::3]:
        check_parts(model, [s])


def test_carry_tile(model):
    for s in ch.carry_cases():
        check_parts(model, [s])


def test_ignorable_runs(model):
    for s in ch.ignorable_runs(1 << 16):
        counts = check_parts(model, [s])
        assert counts[3] == 1 and counts[4] == (s.lower().count(ch.FINAL))


def test_parts(model):
    for data, starts in ch.part_cases():
        rc, got, off, _counts = run_model(model, np.frombuffer(data, np.uint8), np.asarray(starts, np.uint64))
        assert rc == 0
        assert (got, off) == ch.reference(data, starts), (data, starts)


def test_malformed_positions(model):
    for data, starts, pos in [(b"ab\xff", [0], 2), (b"\x80abc", [0], 0), ("\u00e9".encode(), [0, 1], 0), (b"abc\xe2\x82", [0], 3),
                              (b"x" * 4095 + "\u00e9".encode()[:1], [0], 4095), (b"A\xc3\xa9\xed\xa0\x80", [0], 3)]:
        rc, _got, _off, counts = run_model(model, np.frombuffer(data, np.uint8), np.asarray(starts, np.uint64))
        assert rc == -7 and counts[0] == pos, (data, counts)
        with pytest.raises(UnicodeDecodeError) as e:
            cuts = list(starts) + [len(data)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                try:
                    data[a:b].decode("utf-8")
                except UnicodeDecodeError as err:
                    raise UnicodeDecodeError(err.encoding, data, a + err.start, a + err.end, err.reason)
        assert e.value.start == pos
