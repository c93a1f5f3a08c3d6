"""CPU: the rules the windows kernels share with their CPU model (yet-another-bpe_amd/csrc/layout_logic.h: how many rows a
document has, what a row keeps, which source id a slot holds, which document an output row belongs to) run by
tests/hostmodel/windows_model.cpp in the kernels' shape, against the plain-Python contract BBPETokenizer.encode_batch_windows on
synthetic ids -- the grid of tests/test_gpu_encode_windows.py.  The numpy reference that the GPU test uses is held against the
same contract here."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import window_helpers as wh

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libwindows_model.so", HM / "windows_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "layout_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.windows_model.restype = ctypes.c_int
    return lib


def vp(x):
    return ctypes.c_void_p(x.ctypes.data)


def u32(v):
    return ctypes.c_uint32(v or 0)


def model_windows(lib, lens, L, stride, bos, eos, pad_left, piece=4096, with_spans=False):
    """-> (rows, row_doc, row_start, lengths[, spans]), the model's counters"""
    ids, starts = wh.synth(lens)
    n_added = (bos is not None) + (eos is not None)
    cap = wh.win_stats(lens, L, n_added, stride)[0] + 1
    rows, per_row = np.zeros(cap * L, np.uint32), [np.zeros(cap, np.uint32) for _ in range(3)]
    spans, out_spans = wh.synth_spans(len(ids)), np.zeros(cap * L * 2, np.uint64)
    nr, counters = ctypes.c_uint64(0), np.zeros(3, np.uint64)
    flags = (1 if bos is not None else 0) | (2 if eos is not None else 0) | (8 if pad_left else 0)
    rc = lib.windows_model(vp(ids), ctypes.c_uint64(len(ids)), vp(starts), u32(len(lens)), vp(spans) if with_spans else None, u32(L),
                           u32(stride), u32(wh.PAD), u32(bos), u32(eos), u32(flags), u32(piece), vp(rows), vp(per_row[0]), vp(per_row[1]),
                           vp(per_row[2]), vp(out_spans), ctypes.c_uint64(cap), ctypes.byref(nr), vp(counters))
    assert rc == 0
    n = nr.value
    out = (rows[:n * L].reshape(n, L),) + tuple(a[:n] for a in per_row)
    return (out + (out_spans[:n * L * 2].reshape(n, L, 2),) if with_spans else out), counters.tolist()


def same(got, exp, what):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        assert g.shape == e.shape and np.array_equal(g, e), what


def test_windows_grid(model):
    n_cases = 0
    for L, stride, bos, eos, pl in wh.win_cases():
        n_added = (bos is not None) + (eos is not None)
        lens = wh.win_lengths(L, n_added, stride)
        exp = wh.contract_windows(lens, L, stride, wh.PAD, bos, eos, pl)
        ids = wh.synth(lens)[0]
        for piece in (4096, 8, 4):  # small pieces: many of them in a row, many rows in one
            got, counters = model_windows(model, lens, L, stride, bos, eos, pl, piece)
            same(got, exp, (L, stride, bos, eos, pl, piece))
        n_rows, n_multi, n_pad = wh.win_stats(lens, L, n_added, stride)
        assert counters == [max(lens), n_multi, n_rows * L - n_pad] and len(exp[0]) == n_rows
        assert n_pad == int((exp[0] == wh.PAD).sum())  # (the synthetic ids stay below PAD)
        same(wh.np_windows(ids, lens, L, stride, wh.PAD, bos, eos, pl), exp, ("numpy", L, stride, bos, eos, pl))
        n_cases += 1
    assert n_cases > 200


def test_spans_follow_their_ids(model):
    """With spans[i] = (2 i, 2 i + 1) over ids = arange: a content slot that holds id i holds (2 i, 2 i + 1), every other (0, 0)."""
    for L, stride, bos, eos, pl in wh.win_cases():
        n_added = (bos is not None) + (eos is not None)
        lens = wh.win_lengths(L, n_added, stride)
        ids = wh.synth(lens)[0]
        got, _ = model_windows(model, lens, L, stride, bos, eos, pl, 8, with_spans=True)
        exp = wh.np_windows(ids, lens, L, stride, wh.PAD, bos, eos, pl, wh.synth_spans(len(ids)))
        same(got, exp, (L, stride, bos, eos, pl))
        rows, spans = exp[0].astype(np.uint64), exp[4]
        content = rows < wh.PAD
        assert np.array_equal(spans[content], np.stack([2 * rows[content], 2 * rows[content] + 1], axis=1))
        assert not spans[~content].any()


def test_the_rows_of_a_document():
    """The contract's own properties: the row count, full rows but the last, `stride` shared ids, every id covered."""
    for L, stride, bos, eos, pl in wh.win_cases():
        n_added = (bos is not None) + (eos is not None)
        C = L - n_added
        lens = wh.win_lengths(L, n_added, stride)
        _rows, row_doc, row_start, lengths = wh.contract_windows(lens, L, stride, wh.PAD, bos, eos, pl)
        assert np.array_equal(np.bincount(row_doc, minlength=len(lens)), wh.n_rows_of(lens, C, C - stride))
        for d, n in enumerate(lens):
            r = np.flatnonzero(row_doc == d)
            assert np.array_equal(row_start[r], np.arange(len(r)) * (C - stride)) and np.all(lengths[r[:-1]] == L)
            assert row_start[r[-1]] + lengths[r[-1]] - n_added == n  # the last row ends the document
            if len(r) > 1:
                assert n > row_start[r[-2]] + C  # ... and is not contained in the row before


def test_other_paths(model):
    for lens, L, stride, bos, eos in (([20000], 8, 7, None, None), ([1] * 5000, 1, 0, None, None), ([0, 0, 0], 4, 1, 1, None),
                                      ([0], 3, 0, 1, 2), ([7, 8], 8, 3, 1, None)):
        for pl in (False, True):
            exp = wh.contract_windows(lens, L, stride, wh.PAD, bos, eos, pl)
            same(model_windows(model, lens, L, stride, bos, eos, pl)[0], exp, (lens[:3], L, stride))
            same(wh.np_windows(wh.synth(lens)[0], lens, L, stride, wh.PAD, bos, eos, pl), exp, ("numpy", lens[:3], L, stride))
