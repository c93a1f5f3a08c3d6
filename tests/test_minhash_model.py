"""CPU: the MinHash rule the HIP kernels and their CPU model share (yet-another-bpe_amd/csrc/minhash_logic.h), run by
tests/hostmodel/minhash_model.cpp in the kernels' shape -- pieces of 1,024 shingle positions, four waves a piece, passes of 128
functions, minima combined per piece and per document -- against the plain-Python contract BBPETokenizer.minhash_tokens on
the shapes of tests/test_gpu_minhash.py."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import minhash_helpers as mh

HM = Path(__file__).resolve().parent / "hostmodel"


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libminhash_model.so", HM / "minhash_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "minhash_logic.h", csrc / "encode_logic.h", csrc / "pretok_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.minhash_model_run.restype = ctypes.c_longlong
    return lib


def model_run(lib, ids, off, num_perm, ngram, bands, seed=7):
    n_docs, u64, u32, vp = len(off) - 1, ctypes.c_uint64, ctypes.c_uint32, lambda x: ctypes.c_void_p(x.ctypes.data)
    ids1 = np.append(ids, np.uint32(0))  # (never NULL)
    sig, cnt, keys = np.zeros((n_docs, num_perm), np.uint32), np.zeros(n_docs, np.uint64), np.zeros((n_docs, max(bands, 1)), np.uint64)
    rc = lib.minhash_model_run(vp(ids1), u64(len(ids)), vp(off), u32(n_docs), u64(seed), u32(num_perm), u32(ngram), u32(bands), vp(sig), vp(cnt),
                               vp(keys))
    return rc, sig, cnt, keys if bands else None


@pytest.mark.parametrize("num_perm, bands", [(k, 0) for k in mh.PERMS] + list(mh.BANDS))
@pytest.mark.parametrize("ngram", mh.NGRAMS)
def test_model_against_the_contract(model, ngram, num_perm, bands):
    lens = tuple(mh.batch_lengths(ngram))
    exp_sig, exp_cnt, exp_keys = mh.contract(lens, num_perm, ngram, bands or None)
    ids, off = mh.flat(mh.documents(lens))
    rc, sig, cnt, keys = model_run(model, ids, off, num_perm, ngram, bands)
    assert rc == sum(-(-int(c) // mh.TILE) for c in exp_cnt)  # the pieces
    assert np.array_equal(sig, exp_sig) and np.array_equal(cnt, exp_cnt)
    assert keys is None if not bands else np.array_equal(keys, exp_keys)


def test_refused_arguments(model):
    ids, off = mh.flat(mh.documents((3, 9)))
    for bad in ({"num_perm": 0}, {"num_perm": 1025}, {"ngram": 0}, {"ngram": 33}, {"bands": 3}):
        assert model_run(model, ids, off, **{"num_perm": 100, "ngram": 5, "bands": 0, **bad})[0] == -1, bad
