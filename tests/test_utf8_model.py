"""CPU: the rules of errors="replace" / "ignore" on raw text (yet-another-bpe_amd/csrc/utf8_logic.h, the functions the HIP kernels
call) against bytes.decode("utf-8", errors=mode).encode() -- every byte string of length 1 to 4 over one byte of each UTF-8
class as a text of its own and as adjacent parts of one text (the clipping), random longer strings, ill-formed sequences around
a piece edge and a tile edge, and part cuts inside multi-byte characters."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import utf8_helpers as uh

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libutf8_model.so", HM / "utf8_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "utf8_logic.h", csrc / "decode_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.utf8_model.restype = ctypes.c_int
    return lib


def run_model(lib, data: np.ndarray, starts: np.ndarray, mode: str, isolated: bool = False):
    """-> (bytes, offsets list, subparts, first bad position or -1)"""
    data, starts = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(starts, np.uint64)
    cap = 3 * len(data) + 16
    out, off = np.zeros(cap, np.uint8), np.zeros(len(starts) + 1, np.uint64)
    n, counts = ctypes.c_uint64(0), np.zeros(2, np.uint64)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rc = lib.utf8_model(vp(data), ctypes.c_uint64(len(data)), vp(starts), ctypes.c_uint32(len(starts)), ctypes.c_uint32(uh.MODES.get(mode, 0)),
                        ctypes.c_int(int(isolated)), vp(out), ctypes.c_uint64(cap), ctypes.byref(n), vp(off), vp(counts))
    assert rc == 0, rc
    first = int(counts[1])
    return out[:n.value].tobytes(), off.tolist(), int(counts[0]), -1 if first == 2**64 - 1 else first


def check_parts(lib, parts, mode, isolated=False):
    data, starts = uh.pack(parts)
    got = run_model(lib, data, starts, mode, isolated)
    exp = uh.reference(data.tobytes(), starts, mode)
    assert got[1] == exp[1]
    assert got[0] == exp[0]
    assert got[2:] == exp[2:]


def test_sizes(model):
    sizes = np.zeros(3, np.uint32)
    model.utf8_model_sizes(ctypes.c_void_p(sizes.ctypes.data))
    assert sizes.tolist()[:2] == [uh.PIECE, uh.TILE] and sizes[2] >= 3
    assert run_model(model, np.frombuffer(b"a\xffb", np.uint8), np.zeros(1, np.uint64), "replace") == ("a�b".encode(), [0, 5], 1, 1)
    assert run_model(model, np.frombuffer(b"a\xffb", np.uint8), np.zeros(1, np.uint64), "ignore") == (b"ab", [0, 2], 1, 1)


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_every_short_string_alone(model, mode):
    parts = uh.short_strings()
    assert len(parts) > 400_000
    check_parts(model, parts, mode, isolated=True)


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_every_short_string_as_adjacent_parts(model, mode):
    parts = uh.short_strings()
    # the clipping is at work: read as one text, the same bytes give something else
    data, _ = uh.pack(parts[:30_000])
    assert uh.repair(data.tobytes(), mode) != b"".join(uh.repair(p, mode) for p in parts[:30_000])
    check_parts(model, parts, mode)


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_random_long_strings(model, mode):
    parts = uh.random_strings()
    check_parts(model, parts, mode)
    check_parts(model, [b"".join(parts[:2000])], mode)  # ... and as one text


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_sequences_around_a_piece_edge(model, mode):
    seqs = uh.ill_formed_sequences()
    assert len(seqs) > 12_000 and all(uh.ill_formed(s) for s in seqs)
    check_parts(model, uh.edge_cases(uh.PIECE, seqs), mode)


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_sequences_around_a_tile_edge(model, mode):
    parts = uh.edge_cases(uh.TILE, uh.ill_formed_sequences())
    _data, starts = uh.pack(parts)
    assert all(int(s) % uh.TILE == uh.TILE // 2 for s in starts[1:])
    check_parts(model, parts, mode)
    check_parts(model, [b"".join(parts[:5000])], mode)  # one part: nothing is clipped at the edges


@pytest.mark.parametrize("mode", list(uh.MODES))
def test_part_cuts_inside_characters(model, mode):
    cases = uh.cut_cases()
    changed = 0
    for text, starts in cases:
        got = run_model(model, np.frombuffer(text, np.uint8), np.asarray(starts, np.uint64), mode)
        assert got == uh.reference(text, starts, mode), (text, starts)
        changed += got[2] > 0
    assert 0 < changed < len(cases)  # cuts at a character's edge leave it whole


def test_two_handlers_act_on_the_same_ranges():
    for part in uh.random_strings(5000):
        bad = uh.subparts(part)
        assert uh.repair(part, "replace").count("�".encode()) - part.decode("utf-8", "ignore").count("�") == len(bad)
