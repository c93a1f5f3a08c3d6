"""CPU: the masking rule the HIP kernel and its CPU model share (yet-another-bpe_amd/csrc/mask_logic.h), run by
tests/hostmodel/mask_model.cpp in the kernel's shape -- blocks of 256 ids, the document search bounded by the block's ends,
counters reduced per wave and block -- against the plain-Python contract BBPETokenizer.mask_tokens on synthetic ids with
document lengths from lists (no tokenizer model is needed)."""
from __future__ import annotations

import ctypes
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import mask_helpers as mh
from yet_another_bpe.tokenizer import BBPETokenizer

HM = Path(__file__).resolve().parent / "hostmodel"
MASK_ID, N_RANDOM, IGNORE_U32 = 5000, 777, 0xFFFFFF9C
KINDS = ("protected", "masked", "random", "kept")


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libmask_model.so", HM / "mask_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "mask_logic.h", csrc / "encode_logic.h", csrc / "pretok_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.mask_model_run.restype = ctypes.c_int
    return lib


def vp(x):
    return ctypes.c_void_p(x.ctypes.data if x is not None and x.size else 0) if x is not None else ctypes.c_void_p(0)


def model_run(lib, ids, doc_starts, n_docs, words, *, seed=0, first_doc=0, select=0, mask=0, random=0, mask_id=MASK_ID, n_random=N_RANDOM,
              flags=0, block=256):
    n = len(ids)
    out_ids, out_lab, cnt = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(4, np.uint64)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    keep = np.concatenate((words, [0])).astype(np.uint32) if words is not None else None
    words_ptr = ctypes.c_void_p(keep.ctypes.data) if keep is not None else ctypes.c_void_p(0)
    ids1 = np.concatenate((ids, [0])).astype(np.uint32)
    rc = lib.mask_model_run(ctypes.c_void_p(ids1.ctypes.data), u64(n), vp(doc_starts), u32(n_docs), words_ptr, u64(seed), u64(first_doc),
                            u64(select), u64(mask), u64(random), u32(mask_id), u32(n_random), u32(IGNORE_U32), u32(flags), u32(block),
                            ctypes.c_void_p(out_ids.ctypes.data), ctypes.c_void_p(out_lab.ctypes.data), ctypes.c_void_p(cnt.ctypes.data))
    return rc, out_ids[:n], out_lab[:n].view(np.int32), dict(zip(KINDS, cnt.tolist()))


T = BBPETokenizer._dropout_threshold


@pytest.mark.parametrize("name, lens, with_off", mh.LENGTH_SETS, ids=[s[0] for s in mh.LENGTH_SETS])
def test_model_against_the_contract(model, name, lens, with_off):
    tok = BBPETokenizer()
    ids_b, words_b, special_b = mh.synth_batch(lens)
    ids, packed = mh.flat(ids_b, np.uint32), mh.packed_words(words_b, special_b)
    for p, whole_word, seed, first_doc in itertools.product((0, 0.15, 0.5, 1), (False, True), (0, 12345), (0, 1 << 40)):
        for words in ((packed,) if whole_word else (packed, None)):
            exp_in, exp_lab = tok.mask_tokens(ids_b, words_b if words is not None else None, special_b if words is not None else None,
                                              mask_id=MASK_ID, n_random=N_RANDOM, p=p, seed=seed, whole_word=whole_word, first_doc=first_doc)
            rc, got_in, got_lab, cnt = model_run(model, ids, mh.starts(lens) if with_off else None, len(lens), words, seed=seed, first_doc=first_doc,
                                                 select=T(p), mask=T(0.8), random=T(0.1), flags=int(whole_word))
            what = (name, p, whole_word, seed, first_doc, words is not None)
            assert rc == 0, what
            assert got_in.tolist() == [x for r in exp_in for x in r] and got_lab.tolist() == [x for r in exp_lab for x in r], what
            kinds = mh.kinds(ids_b, exp_in, exp_lab, special_b if words is not None else None, MASK_ID)
            n_prot = sum(k == "protected" for r in kinds for k in r)
            assert cnt["protected"] == n_prot and cnt["masked"] + cnt["random"] + cnt["kept"] == sum(x != mh.IGNORE for r in exp_lab for x in r), what
            assert cnt["masked"] == sum(x == MASK_ID for r in exp_in for x in r), what  # (the ids are below 1000)


def test_other_block_sizes_and_fractions(model):
    tok = BBPETokenizer()
    lens = [0, 3, 130, 0, 1, 1, 1, 64, 0]
    ids_b, words_b, special_b = mh.synth_batch(lens, seed=2)
    ids, packed = mh.flat(ids_b, np.uint32), mh.packed_words(words_b, special_b)
    for block, (fm, fr) in itertools.product((64, 128, 256), ((1, 0), (0, 1), (0, 0), (0.5, 0.5))):
        exp_in, exp_lab = tok.mask_tokens(ids_b, words_b, special_b, mask_id=MASK_ID, n_random=N_RANDOM, p=0.5, seed=5, whole_word=True,
                                          mask_fraction=fm, random_fraction=fr)
        rc, got_in, got_lab, _cnt = model_run(model, ids, mh.starts(lens), len(lens), packed, seed=5, select=T(0.5), mask=T(fm), random=T(fr),
                                              flags=1, block=block)
        assert rc == 0 and got_in.tolist() == [x for r in exp_in for x in r] and got_lab.tolist() == [x for r in exp_lab for x in r]


def test_refused_arguments(model):
    ids, st = np.arange(10, dtype=np.uint32), np.asarray([0, 4], np.uint64)
    ok = {"select": T(0.5), "mask": T(0.8), "random": T(0.1)}
    assert model_run(model, ids, st, 2, None, **ok)[0] == 0
    for bad in ({"select": (1 << 32) + 1}, {"mask": (1 << 32) + 1}, {"random": (1 << 32) + 1}, {"mask": T(0.75), "random": T(0.5)}, {"n_random": 0},
                {"flags": 2}, {"flags": 1}):  # (whole-word without words)
        assert model_run(model, ids, st, 2, None, **{**ok, **bad})[0] == -1, bad
    assert model_run(model, ids, st, 2, None, **{**ok, "random": 0, "n_random": 0})[0] == 0
    for starts in ([1, 4], [0, 11], [0, 5, 4]):
        assert model_run(model, ids, np.asarray(starts, np.uint64), len(starts), None, **ok)[0] == -1, starts
    assert model_run(model, ids, None, 2, None, **ok)[0] == -1
