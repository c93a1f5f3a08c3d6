"""CPU: the fill-in-the-middle rule the HIP kernels and their CPU model share (yet-another-bpe_amd/csrc/fim_logic.h), run by
tests/hostmodel/fim_model.cpp in the kernels' shape -- the plan per document, the write per output slot in blocks, the granule
table and the selects for the cuts -- against the plain-Python contract BBPETokenizer.fim_tokens / fim_cuts on the cases of
tests/fim_helpers.py: token level and pieces, block sizes 256, 64 and 1, granules 64 and 4, the counters the call reports,
and every refused argument."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import fim_helpers as fh
from tests import mask_helpers as mh

HM = Path(__file__).resolve().parent / "hostmodel"
COUNTERS = ("n_docs", "n_psm", "n_spm", "n_truncated_docs", "n_ids_dropped", "n_out")
IGNORE = 0xFFFFFF9C
u64, u32 = ctypes.c_uint64, ctypes.c_uint32


@pytest.fixture(scope="module")
def model():
    so, src = HM / "libfim_model.so", HM / "fim_model.cpp"
    csrc = HM.parent.parent / "yet-another-bpe_amd/csrc"
    deps = [src, csrc / "fim_logic.h", csrc / "mask_logic.h", csrc / "encode_logic.h", csrc / "pretok_logic.h"]
    if not so.exists() or so.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.fim_model_run.restype = ctypes.c_int
    lib.fim_model_cuts.restype = ctypes.c_int
    return lib


def ptr(x):
    return ctypes.c_void_p(x.ctypes.data) if x is not None else ctypes.c_void_p(0)


def model_run(lib, ids, doc_starts, n_docs, cuts=None, *, seed=0, first_doc=0, fim=0, spm=0, pre_id=fh.PRE, suf_id=fh.SUF, mid_id=fh.MID, eot_id=None,
              max_len=0, loss_middle=False, pieces=False, flags=0, block=256):
    n = len(ids)
    flags |= (1 if eot_id is not None else 0) | (2 if loss_middle else 0) | (4 if pieces else 0)
    nd = max(n_docs, 1)
    out, lab = np.zeros(n + 4 * nd + 1, np.uint32), np.zeros(n + 4 * nd + 1, np.uint32)
    off, info, cnt = np.zeros(nd + 2, np.uint64), np.zeros(4 * nd + 4, np.uint32), np.zeros(6, np.uint64)
    ids1 = np.concatenate((ids, [0])).astype(np.uint32)
    sent = np.asarray([pre_id, suf_id, mid_id, eot_id or 0], np.uint32)
    cuts = None if cuts is None else np.ascontiguousarray(cuts, np.uint64)
    rc = lib.fim_model_run(ptr(ids1), u64(n), ptr(doc_starts), u32(n_docs), ptr(cuts), u64(seed), u64(first_doc), u64(fim), u64(spm), ptr(sent), u32(IGNORE),
                           u64(max_len), u32(flags), u32(block), ptr(out), ptr(lab), ptr(off), ptr(info), ptr(cnt))
    if rc != 0:
        return rc, None
    n_out_docs = nd // 3 if pieces else nd
    off = off[:n_out_docs + 1]
    return rc, (fh.ragged(out, off), fh.ragged(lab.view(np.int32), off), [tuple(r) for r in info[:4 * n_out_docs].reshape(-1, 4).tolist()],
                dict(zip(COUNTERS, cnt.tolist())))


@pytest.mark.parametrize("index", range(len(fh.cases())), ids=fh.CASE_IDS)
def test_model_against_the_contract(model, index):
    c = fh.cases()[index]
    ids, starts = fh.flat_arrays(index)
    for block in (256, 64, 1):
        rc, got = model_run(model, ids, starts, len(c["lens"]), **fh.native_kwargs(c), block=block)
        assert rc == 0 and got == fh.expected(index), block


@pytest.mark.parametrize("index", range(len(fh.cases())), ids=fh.CASE_IDS)
def test_model_with_pieces(model, index):
    c = fh.cases()[index]
    lens3, cuts, exp = fh.pieces(index)
    ids, _ = fh.flat_arrays(index)
    for block in (256, 64, 1):
        rc, got = model_run(model, ids, mh.starts(lens3), len(lens3), cuts, **fh.native_kwargs(c), pieces=True, block=block)
        assert rc == 0 and got == exp, block


def model_cuts(lib, texts, *, seed=0, first_doc=0, fim=1 << 32, spm=1 << 31, granule=64, starts="given", flags=0, max_len=0):
    blobs = [t.encode("utf-8") for t in texts]
    buf = np.frombuffer(b"".join(blobs) + b"\0", np.uint8)
    st = mh.starts([len(b) for b in blobs]) if isinstance(starts, str) else starts
    po, cu = np.zeros((len(texts), 3), np.uint64), np.zeros((len(texts), 3), np.uint64)
    rc = lib.fim_model_cuts(ptr(buf), u64(len(buf) - 1), ptr(st), u32(len(texts)), u64(seed), u64(first_doc), u64(fim), u64(spm), u64(max_len), u32(flags),
                            u32(granule), ptr(po), ptr(cu))
    return rc, po, cu


@pytest.mark.parametrize("granule", [64, 4])
def test_cuts_against_the_contract(model, granule):
    tok = mh.tokenizer()
    for k, seed, rate in fh.cut_runs():
        texts = fh.CUT_BATCHES[k]
        exp = tok.fim_cuts(texts, fim_rate=rate, spm_rate=0.5, seed=seed, first_doc=3)
        rc, po, cu = model_cuts(model, texts, seed=seed, first_doc=3, fim=fh.threshold(rate), granule=granule)
        assert rc == 0 and [tuple(r) for r in cu.tolist()] == exp, (k, seed)
        assert np.array_equal(po, fh.piece_starts(texts, exp)), (k, seed)


def test_refused_arguments(model):
    ids, st = np.arange(10, dtype=np.uint32), np.asarray([0, 4], np.uint64)
    ok = {"fim": 1 << 31, "spm": 1 << 31}
    assert model_run(model, ids, st, 2, **ok)[0] == 0
    for bad in ({"fim": (1 << 32) + 1}, {"spm": (1 << 32) + 1}, {"max_len": 1}, {"max_len": 3}, {"max_len": 4, "eot_id": 5}, {"flags": 8},
                {"pieces": True}, {"cuts": np.zeros(6, np.uint64)}):  # (pieces: two documents, and no cuts)
        assert model_run(model, ids, st, 2, **{**ok, **bad})[0] == -1, bad
    assert model_run(model, ids, st, 2, **{**ok, "max_len": 4})[0] == 0
    assert model_run(model, ids, st, 2, **{**ok, "max_len": 5, "eot_id": 5})[0] == 0
    assert model_run(model, ids, st, 2, **{**ok, "fim": 1 << 32, "spm": 1 << 32})[0] == 0
    st3 = np.asarray([0, 4, 6], np.uint64)
    assert model_run(model, ids, st3, 3, None, **ok, pieces=True)[0] == -1  # pieces without cuts
    assert model_run(model, ids, st3, 3, np.zeros(3, np.uint64), **ok, pieces=True)[0] == 0
    for starts in ([1, 4], [0, 11], [0, 5, 4]):
        assert model_run(model, ids, np.asarray(starts, np.uint64), len(starts), **ok)[0] == -1, starts
    assert model_run(model, ids, None, 2, **ok)[0] == -1
    assert model_cuts(model, ["ab", "c"], fim=(1 << 32) + 1)[0] == -1
    assert model_cuts(model, ["ab", "c"], flags=8)[0] == -1
    assert model_cuts(model, ["ab", "c"], starts=np.asarray([0, 4], np.uint64))[0] == -1
    assert model_cuts(model, ["ab", "c"], starts=None)[0] == -1
    assert model_cuts(model, ["ab", "c"])[0] == 0
