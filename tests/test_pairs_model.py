"""CPU: Rule 4 of yet-another-bpe_amd/csrc/layout_logic.h (what the two sides of a pair keep, the rows of a pair, what a row keeps,
which source id a slot holds and its type), the code the pairs kernels share with tests/hostmodel/pairs_model.cpp.  (a) its closed
forms against the literal one-id-at-a-time loop, exhaustively; (b) the model, run in the kernels' shape with the piece size as a
parameter, against the plain-Python contract BBPETokenizer.encode_batch_pairs on synthetic ids -- the grid of
tests/test_gpu_encode_pairs.py; (c) the numpy reference that the GPU test uses against the same contract."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import pair_helpers as ph

HM = Path(__file__).resolve().parent / "hostmodel"
MODE = {name: k for k, name in enumerate(ph.MODES)}


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libpairs_model.so", HM / "pairs_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "layout_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.pairs_model.restype = ctypes.c_int
    lib.pairs_keep.restype = None
    return lib


def vp(x):
    return ctypes.c_void_p(x.ctypes.data)


def u32(v):
    return ctypes.c_uint32(v or 0)


def model_pairs(lib, lens, L, mode, stride, bos, eos, sep, n_sep, pad_left, piece=4096, with_spans=False):
    """-> (rows, types, row_pair, row_start, first_len, second_len[, spans]), the model's counters"""
    ids, starts = ph.synth(lens)
    n_sep = n_sep if sep is not None else 0
    cap = len(lens) // 2 + sum(lens) + 1  # (a pair has at most 1 + lb rows)
    rows, types, per_row = np.zeros(cap * L, np.uint32), np.zeros(cap * L, np.uint8), [np.zeros(cap, np.uint32) for _ in range(4)]
    spans, out_spans = ph.synth_spans(len(ids)), np.zeros(cap * L * 2 if with_spans else 2, np.uint64)
    nr, counters = ctypes.c_uint64(0), np.zeros(4, np.uint64)
    flags = (1 if bos is not None else 0) | (2 if eos is not None else 0) | (8 if pad_left else 0)
    rc = lib.pairs_model(vp(ids), ctypes.c_uint64(len(ids)), vp(starts), u32(len(lens)), vp(spans) if with_spans else None, u32(L),
                         u32(MODE[mode]), u32(stride), u32(sep), u32(n_sep), u32(ph.PAD), u32(bos), u32(eos), u32(flags), u32(piece), vp(rows),
                         vp(types), *(vp(a) for a in per_row), vp(out_spans), ctypes.c_uint64(cap), ctypes.byref(nr), vp(counters))
    assert rc == 0
    n = nr.value
    out = (rows[:n * L].reshape(n, L), types[:n * L].reshape(n, L)) + tuple(a[:n] for a in per_row)
    return (out + (out_spans[:n * L * 2].reshape(n, L, 2),) if with_spans else out), counters.tolist()


def same(got, exp, what):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), what


def literal_keep(la, lb, C, mode):
    """the definition: ids leave one at a time"""
    ka, kb = la, lb
    while ka + kb > C:
        if mode == "longest_first":
            first = ka > kb  # (equally long: the second)
        elif mode == "only_first":
            first = ka > 0   # (nothing left: the second alone is longer than C)
        else:
            first = kb == 0
        if first:
            ka -= 1
        else:
            kb -= 1
    return ka, kb


def test_keep_rule_against_the_literal_loop(model):
    """(a) exhaustive over la, lb in 0..12 and C in 1..16, the three truncation modes: the closed forms of Rule 4, numpy's, and the
    contract's own rows"""
    n = 0
    for mode in ph.MODES[:3]:
        for C in range(1, 17):
            grid = [(la, lb) for la in range(13) for lb in range(13)]
            exp = [literal_keep(la, lb, C, mode) for la, lb in grid]
            ka, kb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            for (la, lb), e in zip(grid, exp):
                model.pairs_keep(ctypes.c_uint64(la), ctypes.c_uint64(lb), ctypes.c_uint64(C), u32(MODE[mode]), ctypes.byref(ka), ctypes.byref(kb))
                assert (ka.value, kb.value) == e, (mode, C, la, lb)
                assert sum(e) == min(la + lb, C) and e[0] <= la and e[1] <= lb  # total: the row is full whenever ids were cut
                n += 1
            na, nb = ph.np_keep([g[0] for g in grid], [g[1] for g in grid], C, mode)
            assert list(zip(na.tolist(), nb.tolist())) == exp, (mode, C)
            lens = [x for g in grid for x in g]
            docs = ph.contract_docs(ph.synth(lens)[0], lens)
            out = ph.GivenPairIds().encode_batch_pairs(docs[0::2], docs[1::2], C, truncation=mode, pad_id=ph.PAD)
            assert list(zip(out[4], out[5])) == exp, (mode, C)
    assert n == 3 * 16 * 169


def test_ties_fall_on_the_second():
    assert literal_keep(5, 5, 3, "longest_first") == (2, 1) and literal_keep(5, 5, 4, "longest_first") == (2, 2)
    assert literal_keep(9, 2, 6, "longest_first") == (4, 2) and literal_keep(2, 9, 6, "longest_first") == (2, 4)
    assert literal_keep(9, 9, 4, "only_first") == (0, 4) and literal_keep(9, 9, 4, "only_second") == (4, 0)


def test_pairs_grid(model):
    """(b) and (c) over the grid"""
    n_cases = 0
    for L, mode, stride, bos, eos, sep, n_sep, pl in ph.pair_cases():
        n_added = ph.n_added_of(bos, eos, sep, n_sep)
        lens = ph.pair_lengths(L - n_added, mode, stride)
        exp = ph.contract_pairs(lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl)
        what = (L, mode, stride, bos, eos, sep, n_sep, pl)
        for piece in (4096, 8, 4):  # small pieces: many of them in a row, many rows in one
            got, counters = model_pairs(model, lens, L, mode, stride, bos, eos, sep, n_sep, pl, piece)
            same(got, exp, what + (piece,))
        n_rows, n_cut, n_dropped, n_pad = ph.pair_stats(lens, exp, L, n_added, mode)
        assert counters == [max(lens), n_cut, n_dropped, n_rows * L - n_pad], what
        assert n_pad == int((exp[0] == ph.PAD).sum())  # (the synthetic ids stay below PAD)
        same(ph.np_pairs(ph.synth(lens)[0], lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl), exp, ("numpy",) + what)
        n_cases += 1
    assert n_cases > 400


def test_types_and_spans_follow_their_ids(model):
    """With ids = arange and spans[i] = (2 i, 2 i + 1): a content slot that holds id i holds (2 i, 2 i + 1), every other (0, 0); the
    type of a content slot says which side of its pair id i lies in."""
    for L, mode, stride, bos, eos, sep, n_sep, pl in ph.pair_cases():
        lens = ph.pair_lengths(L - ph.n_added_of(bos, eos, sep, n_sep), mode, stride)
        ids = ph.synth(lens)[0]
        got, _ = model_pairs(model, lens, L, mode, stride, bos, eos, sep, n_sep, pl, 8, with_spans=True)
        exp = ph.np_pairs(ids, lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl, ph.synth_spans(len(ids)))
        same(got, exp, (L, mode, stride, bos, eos, sep, n_sep, pl))
        rows, types, spans = exp[0].astype(np.uint64), exp[1], exp[6]
        content = rows < ph.PAD
        assert np.array_equal(spans[content], np.stack([2 * rows[content], 2 * rows[content] + 1], axis=1))
        assert not spans[~content].any()
        side = np.repeat(np.arange(len(lens)) % 2, lens)  # the side id i lies in
        assert np.array_equal(types[content], side[rows[content]])
        assert np.array_equal(types[~content], (exp[0][~content] == ph.EOS) if eos is not None else np.zeros((~content).sum(), bool))


def test_the_rows_of_a_pair():
    """The contract's own properties in windows mode: every row carries the same head of the first side, the second side's rows
    are those of encode_batch_windows with the slots the first leaves, and every id of the second is covered."""
    for L, mode, stride, bos, eos, sep, n_sep, pl in ph.pair_cases():
        if mode != "windows":
            continue
        n_added = ph.n_added_of(bos, eos, sep, n_sep)
        C = L - n_added
        lens = ph.pair_lengths(C, mode, stride)
        _rows, _types, row_pair, row_start, first_len, second_len = ph.contract_pairs(lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl)
        for p in range(len(lens) // 2):
            la, lb = lens[2 * p], lens[2 * p + 1]
            r = np.flatnonzero(row_pair == p)
            ka = min(la, C - stride - 1)
            Cb = C - ka
            assert len(r) == ph.n_rows_of([lb], Cb, Cb - stride)[0] and np.all(first_len[r] == ka)
            assert np.array_equal(row_start[r], np.arange(len(r)) * (Cb - stride)) and np.all(second_len[r[:-1]] == Cb)
            assert row_start[r[-1]] + second_len[r[-1]] == lb and Cb >= stride + 1


def test_other_paths(model):
    cases = (([0, 20000], 8, "windows", 7, None, None, None, 0),          # step 1: many pieces from one pair
             ([5, 20000], 12, "windows", 3, 1, 2, 3, 2),
             ([1, 1] * 5000, 2, "longest_first", 0, None, None, None, 0),  # more pairs than a count workgroup
             ([1, 1] * 5000, 2, "windows", 0, None, None, None, 0),
             ([3, 9000], 5000, "only_second", 0, 1, 2, 3, 1),              # one row longer than a piece
             ([0, 0, 0, 0, 0, 0], 4, "longest_first", 0, 1, None, 3, 1),   # only empty documents
             ([0, 0], 6, "windows", 1, 1, 2, 3, 2))
    for lens, L, mode, stride, bos, eos, sep, n_sep in cases:
        for pl in (False, True):
            exp = ph.contract_pairs(lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl)
            same(model_pairs(model, lens, L, mode, stride, bos, eos, sep, n_sep, pl)[0], exp, (lens[:3], L, mode, stride))
            same(ph.np_pairs(ph.synth(lens)[0], lens, L, mode, stride, ph.PAD, bos, eos, sep, n_sep, pl), exp, ("numpy", lens[:3], L, mode))
