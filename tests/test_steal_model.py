"""CPU: the arithmetic of the sparse launch's second round (yet-another-bpe_amd/csrc/steal_logic.h) run by
tests/hostmodel/steal_model.cpp -- how the tiles behind the first round of chunks are cut into pieces, and the tagged counter
the workgroups take the pieces from: every piece goes out exactly once under any interleaving of the claimers' atomic
operations (exhaustive for small numbers), whatever an earlier launch left in the counter, and a value read from a word of
another launch's tag is never used."""
from __future__ import annotations

import ctypes
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

HM = Path(__file__).resolve().parent / "hostmodel"
U64, U32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libsteal_model.so", HM / "steal_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "steal_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.steal_piece_tiles.restype = U32
    lib.steal_piece_tiles.argtypes = [U32, U32, U32]
    lib.steal_piece_count.restype = U32
    lib.steal_piece_count.argtypes = [U32, U32]
    lib.steal_arm.restype = U64
    lib.steal_arm.argtypes = [U64]
    lib.steal_claim_all.restype = U32
    lib.steal_claim_all.argtypes = [ctypes.POINTER(U64), U64, U32, ctypes.c_void_p, U32]
    lib.steal_exhaustive.restype = ctypes.c_longlong
    lib.steal_exhaustive.argtypes = [U64, U64, U32, U32]
    lib.steal_schedule.restype = ctypes.c_int
    lib.steal_schedule.argtypes = [U64, U64, U32, U32, ctypes.c_void_p, U32, ctypes.POINTER(U64)]
    return lib


def test_pieces_cover_the_rest_exactly(model):
    rng = random.Random(5)
    cases = [(1, 1, 64), (63, 1, 64), (240_000, 512, 2048), (2048 * 118, 512, 2048), (5, 2048, 2048), (4_000_000_000, 1, 2048)]
    cases += [(rng.randrange(1, 1 << rng.randrange(1, 31)), rng.randrange(1, 2049), 64 * rng.randrange(1, 33)) for _ in range(2000)]
    for rest, blocks, chunk in cases:
        piece = model.steal_piece_tiles(rest, blocks, chunk)
        n = model.steal_piece_count(rest, piece)
        assert piece % 64 == 0 and 64 <= piece <= chunk, (rest, blocks, chunk, piece)
        assert (n - 1) * piece < rest <= n * piece, (rest, blocks, chunk, piece, n)  # no empty piece, nothing left over
        if piece < chunk and piece > 256:  # neither bound reached: one piece per workgroup covers the rest
            assert n <= blocks
    assert model.steal_piece_tiles(2048 * 118, 512, 2048) == 512  # (the flat 1 GiB corpus before its first retile: a quarter chunk each)


@pytest.mark.parametrize("n_claimers", [1, 2, 3])
def test_every_interleaving_hands_each_piece_out_once(model, n_claimers):
    tag = 7
    arm = model.steal_arm
    # what the counter may hold when a launch starts: never used, an older launch's leftovers (also a count far above this
    # launch's number of pieces), and -- a workgroup of THIS launch came first -- this launch's own tag
    starts = [0, arm(6) + 5, arm(1) + 12345, arm(3)]
    for start in starts:
        for n_pieces in range(0, 5 if n_claimers < 3 else 3):
            assert model.steal_exhaustive(start, tag, n_pieces, n_claimers) > 0, (start, n_pieces)


def test_random_interleavings_many_claimers(model):
    rng = random.Random(11)
    for _ in range(300):
        n_claimers, n_pieces = rng.randrange(1, 40), rng.randrange(0, 200)
        tag = rng.randrange(2, 1 << 39)
        start = rng.choice([0, model.steal_arm(rng.randrange(1, tag)) + rng.randrange(0, 1 << 20)])
        sched = np.array([rng.randrange(n_claimers) for _ in range(rng.randrange(0, 3 * (n_pieces + 3 * n_claimers)))], np.uint32)
        word = U64(0)
        assert model.steal_schedule(start, tag, n_pieces, n_claimers, sched.ctypes.data if len(sched) else None, len(sched), ctypes.byref(word)) == 1
        # the word is left with this launch's tag: the next launch's larger tag arms it again
        assert word.value >> 24 == tag and (word.value & 0xFFFFFF) == n_pieces + n_claimers


def test_launch_after_launch_without_clearing(model):
    word = U64(0)
    out = np.zeros(64, np.uint32)
    for tag, n_pieces in [(1, 5), (2, 0), (3, 64), (9, 1), (10, 7)]:
        n = model.steal_claim_all(ctypes.byref(word), tag, n_pieces, out.ctypes.data, 64)
        assert n == n_pieces and out[:n].tolist() == list(range(n_pieces))
    # a stale tag is never claimed from: a claimer of launch 11 that meets launch 10's word does not use its count
    before = word.value
    assert before >> 24 == 10
    assert model.steal_claim_all(ctypes.byref(word), 11, 3, out.ctypes.data, 64) == 3 and out[:3].tolist() == [0, 1, 2]
