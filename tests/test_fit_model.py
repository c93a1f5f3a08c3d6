"""CPU: the rules the whole-document packing shares between the host driver, the HIP kernels and their CPU model
(yet-another-bpe_amd/csrc/fit_logic.h: the plan from the histogram of sequence lengths, the place of a slot), run by
tests/hostmodel/fit_model.cpp in the kernels' shape, against the plain-Python contract BBPETokenizer.encode_batch_fit on synthetic
ids (ids = arange, document lengths from a list: no tokenizer model is needed) and against a literal one-by-one best-fit
decreasing."""
from __future__ import annotations

import ctypes
import random
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from tests import fit_helpers as fh
from tests import layout_helpers as lh

HM = Path(__file__).resolve().parent / "hostmodel"
ROW_LENS = (1, 2, 3, 5, 8, 13, 37, 64)


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libfit_model.so", HM / "fit_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "fit_logic.h", csrc / "layout_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.fit_model_plan.restype = lib.fit_model_rows.restype = ctypes.c_int
    return lib


def vp(x):
    return ctypes.c_void_p(x.ctypes.data)


def u32(v):
    return ctypes.c_uint32(v or 0)


def model_plan(lib, kept, C):
    """-> (first u64[S + 1], place u32[S + 1], places u32[P, 4] = (col, len, rank, per_row), n_rows, steps)"""
    hist = np.bincount(np.asarray(kept, dtype=np.int64), minlength=C + 1).astype(np.uint32)
    cap = len(kept) + 2
    first, place, pl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(4 * cap, np.uint32)
    ns, npl, nr, steps = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.fit_model_plan(vp(hist), u32(C), vp(first), vp(place), vp(pl), u32(cap), u32(cap), ctypes.byref(ns), ctypes.byref(npl),
                            ctypes.byref(nr), ctypes.byref(steps))
    assert rc == 0
    return first[:ns.value + 1], place[:ns.value + 1], pl[:4 * npl.value].reshape(-1, 4), nr.value, steps.value


def model_rows(lib, lens, C, bos, eos, block=256, tile=2048, piece=4096, stage_shapes=256, stage_places=1024):
    ids, starts = lh.synth(lens)
    n_added = (bos is not None) + (eos is not None)
    cap_rows = len(lens) + 1
    cap = cap_rows * C
    out = [np.zeros(cap, np.uint32) for _ in range(3)]
    used, order, nr = np.zeros(cap_rows, np.uint32), np.zeros(max(len(lens), 1), np.uint32), ctypes.c_uint64(0)
    rc = lib.fit_model_rows(vp(ids), ctypes.c_uint64(len(ids)), vp(starts), u32(len(lens)), u32(C), u32(lh.PAD), u32(bos), u32(eos),
                            u32(fh.flags_of(bos, eos)), u32(block), u32(tile), u32(piece), u32(stage_shapes), u32(stage_places), vp(out[0]),
                            vp(out[1]), vp(out[2]), vp(used), ctypes.c_uint64(cap), ctypes.c_uint64(cap_rows), vp(order), ctypes.byref(nr))
    assert rc == 0
    if nr.value:  # the sort the write read: stable by n_d
        kept = np.asarray(fh.kept_lengths(lens, C, n_added))
        assert order[:len(lens)].tolist() == np.argsort(kept, kind="stable").tolist()
    return tuple(a[:nr.value * C].reshape(nr.value, C) for a in out) + (used[:nr.value],)


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.shape == e.shape and np.array_equal(g, e), what


def random_lengths(rng, C):
    """content lengths: uniform, or clustered on a few values; now and then empty and over-long documents"""
    n = rng.choice([0, 1, 2, 5, 30, 200])
    if rng.random() < 0.5:
        lens = [rng.randint(0, C + 2) if rng.random() < 0.1 else rng.randint(1, C) for _ in range(n)]
    else:
        few = [1, max(1, C // 3), max(1, C // 2), C, rng.randint(1, C)]
        lens = [rng.choice(few) for _ in range(n)]
    return lens


def test_plan_against_the_contract_and_literal_bfd(model):
    rng = random.Random(1)
    for trial in range(2000):
        C = rng.choice(ROW_LENS)
        bos, eos = rng.choice(lh.ADDED)
        n_added = (bos is not None) + (eos is not None)
        if C < max(1, n_added):
            continue
        lens = random_lengths(rng, C)
        kept = fh.kept_lengths(lens, C, n_added)
        what = (trial, C, bos, eos, lens)
        first, place, pl, n_rows, _steps = model_plan(model, kept, C)
        _ids, doc, pos, used = fh.contract(lens, C, bos, eos)
        # the model's shapes, row by row, are the contract's
        shapes = [tuple(pl[place[s]:place[s + 1], 1].tolist()) for s in range(len(first) - 1) for _ in range(int(first[s + 1] - first[s]))]
        assert len(shapes) == n_rows and shapes == fh.row_shapes(doc, pos), what
        assert used.tolist() == [sum(s) for s in shapes], what
        distinct = [tuple(pl[place[s]:place[s + 1], 1].tolist()) for s in range(len(first) - 1)]
        assert distinct == sorted(set(distinct), reverse=True), what  # each shape once, in descending tuple order
        # no row over C, shapes non-increasing, places end to end from column 0
        for s in range(len(first) - 1):
            p = pl[place[s]:place[s + 1]]
            assert len(p) and p[:, 1].sum() <= C and np.all(np.diff(p[:, 1].astype(np.int64)) <= 0), what
            assert p[:, 0].tolist() == (np.cumsum(p[:, 1]) - p[:, 1]).tolist(), what
        # every document is placed exactly once, at a place of its length
        order = np.argsort(np.asarray(kept, dtype=np.int64), kind="stable")
        taken = []
        for s in range(len(first) - 1):
            for col, length, rank, per_row in pl[place[s]:place[s + 1]].tolist():
                for i in range(int(first[s + 1] - first[s])):
                    taken.append(rank + i * per_row)
                    assert kept[order[rank + i * per_row]] == length, what
        n_empty = kept.count(0)
        assert sorted(taken) == list(range(n_empty, len(kept))), what
        # the rooms are those of best-fit decreasing one sequence at a time; at most one row is at most half full
        assert Counter(C - sum(s) for s in shapes) == fh.literal_rooms(kept, C), what
        assert sum(1 for s in shapes if 2 * sum(s) <= C) <= 1, what


def test_hand_example(model):
    """C = 10, lengths 6, 6, 6, 2, 2, 2: rows (6, 2, 2), (6, 2), (6): documents 0, 3, 4 / 1, 5 / 2."""
    first, place, pl, n_rows, steps = model_plan(model, [6, 6, 6, 2, 2, 2], 10)
    assert n_rows == 3 and first.tolist() == [0, 1, 2, 3] and place.tolist() == [0, 3, 5, 6]
    assert pl.tolist() == [[0, 6, 3, 1], [6, 2, 0, 2], [8, 2, 1, 2], [0, 6, 4, 1], [6, 2, 2, 1], [0, 6, 5, 1]]
    _ids, doc, _pos, used = model_rows(model, [6, 6, 6, 2, 2, 2], 10, None, None)
    assert doc.tolist() == [[0] * 6 + [3] * 2 + [4] * 2, [1] * 6 + [5] * 2 + [lh.NO_DOC] * 2, [2] * 6 + [lh.NO_DOC] * 4]
    assert used.tolist() == [10, 8, 6]


def test_slots_in_the_kernel_shape(model):
    """fit_slot over every (row, col): the four arrays of the contract, with the kernel's sizes and with pieces and windows
    small enough that most pieces overflow theirs."""
    rng = random.Random(2)
    shapes_of_run = ({}, {"piece": 8, "stage_shapes": 1, "stage_places": 2, "block": 64, "tile": 128},
                     {"piece": 16, "stage_shapes": 2, "stage_places": 3, "block": 128, "tile": 128})
    for trial in range(600):
        C = rng.choice(ROW_LENS)
        bos, eos = rng.choice(lh.ADDED)
        if C < max(1, (bos is not None) + (eos is not None)):
            continue
        lens = random_lengths(rng, C)
        same(model_rows(model, lens, C, bos, eos, **shapes_of_run[trial % 3]), fh.contract(lens, C, bos, eos), (trial, C, bos, eos, lens))


def test_other_paths(model):
    rng = np.random.default_rng(3)
    cases = [
        ("more than one piece, rows not aligned to 4", rng.integers(1, 41, 700).tolist(), 37, None, 70002),
        ("more places in a piece than the stage holds", [1] * 6000 + [2] * 40, 5000, None, None),
        ("a second radix digit", rng.integers(1, 301, 1500).tolist(), 300, None, None),
        ("equal keys", [3] * 1000, 10, None, None),
        ("longer than the row", [50, 3, 0, 41, 40, 39, 38], 40, 70001, 70002),
        ("row_len == n_added", [0, 4, 1, 0], 2, 70001, 70002),
        ("only empty documents", [0, 0, 0], 8, None, None),
        ("one full row", [8], 8, None, None),
    ]
    for name, lens, C, bos, eos in cases:
        same(model_rows(model, lens, C, bos, eos), fh.contract(lens, C, bos, eos), name)
    first, place, _pl, _n, _steps = model_plan(model, [1] * 6000 + [2] * 40, 5000)
    assert max(np.diff(place.astype(np.int64))) > 1024  # (that case does leave the kernel's stage)
