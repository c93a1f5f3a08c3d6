"""CPU: NFC normalisation (yet-another-bpe_amd/csrc/nfc_logic.h, the functions the k_nfc_* kernels call, run by
tests/hostmodel/nfc_model.cpp in the kernels' steps with the kernels' window, piece and short-buffer sizes) against
unicodedata.normalize("NFC", part) of this interpreter: the generated tables code point by code point, every single code
point, every pair of the composition table, every Hangul syllable, 200,000 random strings over the code points that can
change anything, dirty segments against the window and carry edges, segments around the short buffer's size and the cap,
parts that begin with a mark, empty parts, a part cut inside a dirty segment."""
from __future__ import annotations

import ctypes
import subprocess
import unicodedata as ud
from pathlib import Path

import numpy as np
import pytest

from tests import nfc_helpers as nh

HM = Path(__file__).resolve().parent / "hostmodel"
CSRC = HM.parent.parent / "yet-another-bpe_amd/csrc"
E_CAPACITY, E_UTF8 = -4, -7


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libnfc_model.so", HM / "nfc_model.cpp"
    deps = [src, CSRC / "nfc_logic.h", CSRC / "pretok_logic.h", CSRC / "tile_logic.h", CSRC / "unicode_norm.inc"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.nfc_model.restype = ctypes.c_int
    lib.nfc_model_version.restype = ctypes.c_char_p
    lib.nfc_model_prop.restype = ctypes.c_uint32
    lib.nfc_model_compose.restype = ctypes.c_uint32
    lib.nfc_model_n_pairs.restype = ctypes.c_uint32
    lib.nfc_model_const.restype = ctypes.c_uint64
    return lib


def run(lib, data, starts=(0,)):
    """-> (rc, normalised bytes, offsets, bad_pos, stats dict)"""
    text = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    n = len(data)
    st = np.ascontiguousarray(starts, dtype=np.uint64)
    out = np.zeros(3 * n + 1, dtype=np.uint8)
    off = np.zeros(len(st) + 1, dtype=np.uint64)
    n_out, bad = ctypes.c_uint64(0), ctypes.c_int64(-1)
    stats = np.zeros(4, dtype=np.uint64)
    vp = ctypes.c_void_p
    rc = lib.nfc_model(vp(text.ctypes.data), ctypes.c_uint64(n), vp(st.ctypes.data), ctypes.c_uint32(len(st)), vp(out.ctypes.data),
                       vp(off.ctypes.data), ctypes.byref(n_out), ctypes.byref(bad), vp(stats.ctypes.data))
    return rc, out[:n_out.value].tobytes(), off.tolist(), bad.value, dict(zip(("suspects", "dirty", "long", "copied"), stats.tolist()))


def check_parts(lib, strings):
    """the strings as parts of one buffer against unicodedata: bytes and offsets"""
    buf, starts = nh.pack(strings)
    rc, got, off, _bad, stats = run(lib, buf.tobytes(), starts if len(starts) else (0,))
    exp, exp_off = nh.reference(buf.tobytes(), starts if len(starts) else (0,))
    assert rc == 0
    if got != exp or off != exp_off:  # name the first part that differs
        for k, s in enumerate(strings):
            a = got[off[k]:off[k + 1]]
            assert a == exp[exp_off[k]:exp_off[k + 1]], (k, [hex(ord(c)) for c in (s if isinstance(s, str) else s.decode())][:40], a[:60])
        assert off == exp_off
    return stats


def test_constants_and_version(model):
    assert [model.nfc_model_const(k) for k in range(4)] == [nh.WIN, nh.PIECE, nh.SHORT, nh.CAP]
    assert model.nfc_model_const(6) == nh.CARRY_TILE
    assert model.nfc_model_version().decode() == ud.unidata_version, \
        "csrc/unicode_norm.inc was generated from another Unicode version: rerun tools/gen_unicode_norm.py"


def test_tables_match_unicodedata(model):
    maybe, no = nh.quick_check_sets()
    assert (len(maybe), len(no)) == (111, 1120) and not set(maybe) & set(no)
    maybe, no = set(maybe), set(no)
    first, first_decomp = model.nfc_model_const(4), model.nfc_model_const(5)
    n_decomp = 0
    out = (ctypes.c_uint32 * 4)()
    for cp in nh.code_points():
        ch = chr(cp)
        p = model.nfc_model_prop(cp)
        assert p & 0xFF == ud.combining(ch), hex(cp)
        assert p >> 8 == (2 if cp in no else 1 if cp in maybe else 0), hex(cp)
        assert p == 0 or cp >= first, hex(cp)
        k = model.nfc_model_decompose(cp, out)
        full = [ord(x) for x in ud.normalize("NFD", ch)]
        assert list(out[:k]) == full, hex(cp)
        assert full == [cp] or cp >= first_decomp, hex(cp)
        n_decomp += full != [cp] and not 0xAC00 <= cp < 0xAC00 + 11172
    assert n_decomp == 2061


def test_every_code_point_and_every_pair(model):
    cps = nh.code_points()
    for lo in range(0, len(cps), 50000):
        check_parts(model, [chr(cp) for cp in cps[lo:lo + 50000]])
    n = model.nfc_model_n_pairs()
    assert n == 941
    row = (ctypes.c_uint32 * 3)()
    pairs = []
    for i in range(n):
        model.nfc_model_pair(i, row)
        a, b, c = row
        assert nh.nfc(chr(a) + chr(b)) == chr(c) and model.nfc_model_compose(a, b) == c
        pairs.append(chr(a) + chr(b))
    assert pairs == sorted(pairs, key=lambda s: (ord(s[0]), ord(s[1])))
    check_parts(model, pairs)
    assert model.nfc_model_compose(0x61, 0x62) == 0 and model.nfc_model_compose(0x0308, 0x0301) == 0


def test_hangul(model):
    syl = [chr(cp) for cp in range(0xAC00, 0xAC00 + 11172)]
    stats = check_parts(model, [ud.normalize("NFD", s) for s in syl])
    assert stats["dirty"] == 11172
    assert check_parts(model, syl)["suspects"] == 0


def test_random_strings(model):
    strings = nh.random_strings(23, 200_000)
    nh.assert_kinds(strings)
    for lo in range(0, len(strings), 20_000):
        check_parts(model, strings[lo:lo + 20_000])
    # ... and as ONE part each way of cutting it would be another text: a few long concatenations
    for lo in range(0, 2_000, 100):
        check_parts(model, ["".join(strings[lo:lo + 100])])


def test_segment_rule(model):
    """A segment the rule calls clean is one NFC leaves alone: no suspect <=> unchanged, on the random strings' segments."""
    for s in nh.random_strings(29, 5_000) + nh.DIRTY:
        rc, got, _off, _bad, stats = run(model, s.encode())
        assert rc == 0 and got == nh.nfc(s).encode()
        if stats["suspects"] == 0:
            assert nh.nfc(s) == s and stats["copied"] == 0
        if nh.nfc(s) != s:
            assert stats["dirty"] >= 1


def test_window_edges(model):
    check_parts(model, nh.edge_cases())
    for s in nh.edge_cases()[::5]:
        check_parts(model, [s])


def test_carry_edge(model):
    for s in nh.carry_cases():
        assert check_parts(model, [s])["dirty"] == 12


def test_short_buffer_and_long_path(model):
    for s in nh.length_cases():
        stats = check_parts(model, [s])
        assert stats["dirty"] >= 1, s[:8]
    # 31 / 32 / 33 decomposed code points in one segment: the last one takes the long path
    for n, long in ((nh.SHORT - 1, 0), (nh.SHORT, 0), (nh.SHORT + 1, 1)):
        assert check_parts(model, ["a" + "\u0301" * (n - 1)])["long"] == long
        assert check_parts(model, ["\u1e09" + "\u0323" * (n - 3)])["long"] == long  # U+1E09 decomposes into three
    assert check_parts(model, nh.length_cases())["long"] >= 8


def test_cap(model):
    at = "a" + "\u0301" * (nh.CAP - 1)
    stats = check_parts(model, ["xy", at, "z"])
    assert stats["long"] == 1
    over = ("xy" + "a" + "\u0301" * nh.CAP + "z").encode()
    rc, _got, _off, bad, _stats = run(model, over)
    assert rc == E_CAPACITY and bad == 2
    # a clean segment has no cap: U+0591 has ccc 220 and quick-check Yes
    stats = check_parts(model, ["\u0591" * (4 * nh.CAP)])
    assert stats["suspects"] == 0 and stats["copied"] == 0


def test_parts(model):
    for data, starts in nh.part_cases():
        rc, got, off, _bad, _stats = run(model, data, starts)
        exp, exp_off = nh.reference(data, starts)
        assert rc == 0 and got == exp and off == exp_off, (data, starts, got, exp, off, exp_off)


def test_malformed_utf8(model):
    for data, starts in [(b"ab\xffcd", (0,)), (b"e\xcc", (0,)), ("a\u0301".encode(), (0, 2)), (b"\x80", (0,)), (b"ok\xed\xa0\x80", (0,)),
                         ("x\u00e9".encode() * 3000 + b"\xc3", (0,))]:
        rc, _got, _off, bad, _stats = run(model, data, starts)
        cuts = list(starts) + [len(data)]
        exp = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            try:
                data[a:b].decode("utf-8")
            except UnicodeDecodeError as e:
                exp = a + e.start
                break
        assert rc == E_UTF8 and bad == exp, (data[:20], starts, bad, exp)
