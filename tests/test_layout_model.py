"""CPU: the index rules the layout kernels share with their CPU model (yet-another-bpe_amd/csrc/layout_logic.h: which source id
a padded slot holds, which document and position a stream position belongs to) run by tests/hostmodel/layout_model.cpp in the
kernels' shape, against the plain-Python contract BBPETokenizer.encode_batch_padded / encode_batch_packed on synthetic ids
(ids = arange, document lengths from a list: no tokenizer model is needed) -- the length grid of tests/test_gpu_encode_layout.py.
The numpy references that the GPU test uses are held against the same contract here."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import layout_helpers as lh

HM = Path(__file__).resolve().parent / "hostmodel"
TOK = lh.GivenIds()
FLAGS = {"bos": 1, "eos": 2, "trunc_left": 4, "pad_left": 8, "drop_last": 16}


@pytest.fixture(scope="module")
def model():
    so, src = HM / "liblayout_model.so", HM / "layout_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "layout_logic.h", csrc / "tile_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.layout_model_pad.restype = lib.layout_model_pack.restype = ctypes.c_int
    return lib


def vp(x):
    return ctypes.c_void_p(x.ctypes.data)


def u32(v):
    return ctypes.c_uint32(v or 0)


def flags_of(bos, eos, **kw):
    return (1 if bos is not None else 0) | (2 if eos is not None else 0) | sum(FLAGS[k] for k, on in kw.items() if on)


def model_pad(lib, lens, L, bos, eos, trunc_left, pad_left):
    ids, starts = lh.synth(lens)
    cap = (max(lens, default=0) + 2) * len(lens) if not L else L * len(lens)
    rows, out_len, rl = np.zeros(cap + 1, np.uint32), np.zeros(len(lens), np.uint32), ctypes.c_uint32(0)
    rc = lib.layout_model_pad(vp(ids), ctypes.c_uint64(len(ids)), vp(starts), u32(len(lens)), u32(L), u32(lh.PAD), u32(bos), u32(eos),
                              u32(flags_of(bos, eos, trunc_left=trunc_left, pad_left=pad_left)), vp(rows), ctypes.c_uint64(cap), vp(out_len),
                              ctypes.byref(rl))
    assert rc == 0
    return rows[:len(lens) * rl.value].reshape(len(lens), rl.value), out_len


def model_pack(lib, lens, L, bos, eos, drop_last, piece=4096, stage=2048):
    ids, starts = lh.synth(lens)
    cap = len(ids) + 2 * len(lens) + L
    out = [np.zeros(cap, np.uint32) for _ in range(3)]
    nr = ctypes.c_uint64(0)
    rc = lib.layout_model_pack(vp(ids), ctypes.c_uint64(len(ids)), vp(starts), u32(len(lens)), u32(L), u32(lh.PAD), u32(bos), u32(eos),
                               u32(flags_of(bos, eos, drop_last=drop_last)), u32(piece), u32(stage), vp(out[0]), vp(out[1]), vp(out[2]),
                               ctypes.c_uint64(cap), ctypes.byref(nr))
    assert rc == 0
    return tuple(a[:nr.value * L].reshape(nr.value, L) for a in out)


def contract_pad(lens, L, bos, eos, trunc_left, pad_left):
    ids, _ = lh.synth(lens)
    rows, kept = TOK.encode_batch_padded(lh.contract_docs(ids, lens), L, pad_id=lh.PAD, bos_id=bos, eos_id=eos,
                                         truncation="left" if trunc_left else "right", padding_side="left" if pad_left else "right")
    return np.asarray(rows, dtype=np.uint32).reshape(len(lens), -1), np.asarray(kept, dtype=np.uint32)


def contract_pack(lens, L, bos, eos, drop_last):
    ids, _ = lh.synth(lens)
    out = TOK.encode_batch_packed(lh.contract_docs(ids, lens), L, pad_id=lh.PAD, bos_id=bos, eos_id=eos, drop_last=drop_last)
    return tuple(np.asarray(a, dtype=np.uint32).reshape(-1, L) for a in out)


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.shape == e.shape and np.array_equal(g, e), what


def test_padded_grid(model):
    for L, bos, eos, tl, pl in lh.pad_cases():
        lens = lh.grid_lengths(L, (bos is not None) + (eos is not None))
        exp = contract_pad(lens, L, bos, eos, tl, pl)
        same(model_pad(model, lens, L, bos, eos, tl, pl), exp, (L, bos, eos, tl, pl))
        same(lh.np_pad(lh.synth(lens)[0], lens, L, lh.PAD, bos, eos, tl, pl), exp, ("numpy", L, bos, eos, tl, pl))


def test_packed_grid(model):
    for L, bos, eos, dl in lh.pack_cases():
        lens = lh.grid_lengths(L, (bos is not None) + (eos is not None))
        exp = contract_pack(lens, L, bos, eos, dl)
        for piece, stage in ((4096, 2048), (8, 4), (4, 2)):  # small pieces: many windows, with and without the stage
            same(model_pack(model, lens, L, bos, eos, dl, piece, stage), exp, (L, bos, eos, dl, piece))
        same(lh.np_pack(lh.synth(lens)[0], lens, L, lh.PAD, bos, eos, dl), exp, ("numpy", L, bos, eos, dl))


def test_longest_sequence_as_row_length(model):
    for bos, eos in lh.ADDED:
        for lens in ([3, 0, 11, 5], [0, 0], [0], [1]):
            exp = contract_pad(lens, None, bos, eos, False, True)
            assert exp[0].shape[1] == max(lens) + (bos is not None) + (eos is not None)
            same(model_pad(model, lens, 0, bos, eos, False, True), exp, (lens, bos, eos))
            same(lh.np_pad(lh.synth(lens)[0], lens, None, lh.PAD, bos, eos, False, True), exp, ("numpy", lens, bos, eos))


def test_other_paths(model):
    for name, lens in lh.special_length_sets().items():
        for (bos, eos), L in ((lh.ADDED[0], 64), (lh.ADDED[2], 33), (lh.ADDED[3], 2048)):
            for dl in (False, True):
                exp = contract_pack(lens, L, bos, eos, dl)
                same(model_pack(model, lens, L, bos, eos, dl), exp, (name, L, dl))
                same(lh.np_pack(lh.synth(lens)[0], lens, L, lh.PAD, bos, eos, dl), exp, ("numpy", name, L, dl))
            exp = contract_pad(lens, L, bos, eos, True, False)
            same(model_pad(model, lens, L, bos, eos, True, False), exp, (name, L))
            same(lh.np_pad(lh.synth(lens)[0], lens, L, lh.PAD, bos, eos, True, False), exp, ("numpy", name, L))
    lens = [64] * 8  # a stream that is an exact multiple of the row: no pad slot
    ids, doc, pos = model_pack(model, lens, 128, None, None, False)
    assert ids.shape == (4, 128) and not (doc == lh.NO_DOC).any()
    same((ids, doc, pos), contract_pack(lens, 128, None, None, False), "exact multiple")
    assert model_pack(model, [0, 0], 8, None, None, False)[0].shape == (0, 8)  # a stream of length 0: zero rows
