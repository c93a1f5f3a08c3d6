"""CPU: the placement rules of the tile-centric loader (yet-another-bpe_amd/csrc/load_logic.h) run by
tests/hostmodel/load_model.cpp -- the kernel's steps (K-ary search for a run's first word, forward walk, byte window in
aligned pieces, one lane per word) against the straightforward per-word loop: the first word of every tile, every slot of
every tile, tile lengths, word bases and the long-word list, in both layouts; and the same model as a stand-alone program
under AddressSanitizer and UBSan."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import load_cases

HM = Path(__file__).resolve().parent / "hostmodel"
CSRC = HM.parent.parent / "yet-another-bpe_amd" / "csrc"
DEPS = [HM / "load_model.cpp", CSRC / "load_logic.h", CSRC / "tile_logic.h"]
U64, U32 = ctypes.c_uint64, ctypes.c_uint32


def _stale(out: Path) -> bool:
    return not out.exists() or out.stat().st_mtime < max(d.stat().st_mtime for d in DEPS)


@pytest.fixture(scope="module")
def model():
    so = HM / "libload_model.so"
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(DEPS[0])])
    lib = ctypes.CDLL(str(so))
    lib.load_model_n_tiles.restype = U64
    lib.load_model_n_tiles.argtypes = [ctypes.c_void_p, U64]
    args = [ctypes.c_void_p, ctypes.c_void_p, U64, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.POINTER(U64)] * 2
    lib.load_model_per_word.restype = None
    lib.load_model_per_word.argtypes = args
    lib.load_model_tiled.restype = ctypes.c_int
    lib.load_model_tiled.argtypes = args
    lib.retile_model_new_n.restype = U64
    lib.retile_model_new_n.argtypes = [ctypes.c_void_p, U64]
    lib.retile_model_scatter.restype = None
    lib.retile_model_scatter.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, U64]
    lib.retile_model_gather.restype = ctypes.c_int
    lib.retile_model_gather.argtypes = [ctypes.c_void_p, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, U64, U32]
    return lib


def run(model, fn, flat, off, weighted):
    n = len(off) - 1
    nt = model.load_model_n_tiles(off.ctypes.data, n)
    tiles = np.zeros((nt, load_cases.CAP), np.uint16)
    tlen, wbase, first = (np.zeros(nt, np.uint32) for _ in range(3))
    longs = np.zeros(n + 1, np.uint32)
    n_long, long_tokens = U64(0), U64(0)
    keep = np.concatenate([flat, np.zeros(1, np.uint8)])  # (a valid address for an empty corpus)
    rc = fn(keep.ctypes.data, off.ctypes.data, n, weighted, tiles.ctypes.data, tlen.ctypes.data, wbase.ctypes.data, first.ctypes.data,
            longs.ctypes.data, ctypes.byref(n_long), ctypes.byref(long_tokens))
    assert not rc, rc
    if not weighted:
        wbase[:] = 0xFFFFFFFF  # (no word bases in the flat layout)
    return {"tiles": tiles, "tile_len": tlen, "tile_wbase": wbase, "first": first, "long": np.sort(longs[:n_long.value]), "long_tokens": long_tokens.value}


def compare(model, flat, off, weighted):
    a = run(model, model.load_model_per_word, flat, off, weighted)
    b = run(model, model.load_model_tiled, flat, off, weighted)
    assert np.array_equal(a["first"], b["first"])  # the first word of every tile
    assert np.array_equal(a["tiles"], b["tiles"])  # the slot of every element (and PAD everywhere else)
    for k in ("tile_len", "tile_wbase", "long"):
        assert np.array_equal(a[k], b[k]), k
    assert a["long_tokens"] == b["long_tokens"]
    return a


@pytest.mark.parametrize("weighted", [0, 1])
@pytest.mark.parametrize("name", list(load_cases.cases()))
def test_tiled_placement_equals_per_word_loop(model, name, weighted):
    lens, off_base = load_cases.cases()[name]
    flat, off = load_cases.build(lens, off_base)
    a = compare(model, flat, off, weighted)
    S = load_cases.SPAN
    if name == "longer_than_a_span":
        assert a["first"].tolist() == [0, 0xFFFFFFFF, 2] and a["tile_len"][1] == 0 and (a["tiles"][1] == 0xFFFE).all()
    if name == "ends_on_last_span_slot":
        assert a["tiles"][0, S - 1] == 0xFFFF and a["first"][1] == 2
    if name == "starts_on_slot_span_minus_1":
        assert a["tile_len"][0] == load_cases.CAP and a["tiles"][0, load_cases.CAP - 1] == 0xFFFF and a["first"][1] == 3
    if name == "lengths_0_1_2_63_64":
        assert a["long"].tolist() == [4, 8]
        assert a["tile_len"][0] == 273 and a["tiles"][0, 0] == (0xFFFF if weighted else 0xFFFE)  # (the last word starts on packed position 270)


def test_random_corpora(model):
    rng = random.Random(17)
    for _ in range(60):
        hi = rng.choice([3, 12, 70, 300])
        lens = [rng.randrange(0, hi) if rng.random() > 0.002 else rng.randrange(900, 3000) for _ in range(rng.randrange(1, 6000))]
        flat, off = load_cases.build(lens, rng.randrange(0, 50))
        compare(model, flat, off, rng.randrange(2))


def retile_compare(model, tiles_words: list[list[int]], group: int = 8):
    """tiles_words[t]: the kept words of old tile t, as lengths with their SEP"""
    n_of = np.array([len(t) for t in tiles_words] + [0], np.uint32)
    wlen = np.array([L for t in tiles_words for L in t] + [0], np.uint32)
    n_tiles, n_w = len(tiles_words), len(wlen) - 1
    new_n = model.retile_model_new_n(wlen.ctypes.data, n_w)
    out = []
    for gather in (False, True):
        tiles, tlen = np.zeros((new_n, load_cases.CAP), np.uint16), np.zeros(new_n, np.uint32)
        if gather:
            assert model.retile_model_gather(n_of.ctypes.data, n_tiles, wlen.ctypes.data, tiles.ctypes.data, tlen.ctypes.data, new_n, group) == 0
        else:
            model.retile_model_scatter(n_of.ctypes.data, n_tiles, wlen.ctypes.data, tiles.ctypes.data, tlen.ctypes.data, new_n)
        out.append((tiles, tlen))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])
    return out[1]


def test_gathering_retile_places_every_element_like_the_scatter(model):
    S = load_cases.SPAN
    retile_compare(model, [[]])  # nothing kept: one empty tile
    tiles, tlen = retile_compare(model, [[], [], []])
    assert tlen.tolist() == [0] and (tiles == 0xFFFE).all()
    retile_compare(model, [[3]])
    retile_compare(model, [[S - 3, 3], [64, 2]])          # a word ends on the last slot of the span; the next tile starts at slot 0
    tiles, tlen = retile_compare(model, [[S - 1, 64], [5]])  # a 64-slot word from slot SPAN-1 fills the LMAX tail
    assert tlen.tolist() == [load_cases.CAP, 64 - 1 + 5] and (tiles[1, :63] == 0xFFFE).all()
    rng = random.Random(23)
    for _ in range(40):
        old = []
        for _t in range(rng.randrange(1, 400)):
            room, words = (0 if rng.random() < 0.2 else rng.randrange(0, load_cases.CAP + 1)), []
            while room >= 2:
                L = min(room, rng.randrange(2, 65))
                words.append(L)
                room -= L
            old.append(words)
        retile_compare(model, old, rng.choice([1, 2, 8]))


def test_model_under_sanitizers(tmp_path):
    exe = tmp_path / "load_model_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DLOAD_MODEL_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), str(DEPS[0])])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
