"""GPU: yabpe_fim bit for bit against the plain-Python BBPETokenizer.fim_tokens on the cases of tests/fim_helpers.py (the
list the CPU model runs), at token level and with pieces, inputs as host arrays and as device memory: sequences, labels,
offsets, info and the call's statistics; results that outlive later encode, mask, span and layout calls, yabpe_fim_free
and a second call; and every refused argument, each before anything is allocated."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import fim_helpers as fh
from tests import mask_helpers as mh

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
COUNTERS = ("n_docs", "n_psm", "n_spm", "n_truncated_docs", "n_ids_dropped", "n_out")


@pytest.fixture(scope="module")
def tok():
    return mh.tokenizer()


def as_lists(got):
    ids, labels, off, info = got
    assert (ids.dtype, labels.dtype, off.dtype, info.dtype) == (np.uint32, np.int32, np.uint64, np.uint32)
    assert off[0] == 0 and off[-1] == len(ids) == len(labels) and info.shape == (len(off) - 1, 4)
    return fh.ragged(ids, off), fh.ragged(labels, off), [tuple(r) for r in info.tolist()]


def device_copy(ctx, ids, starts):
    """the ids in device memory: a mask that selects nothing copies them there"""
    return ctx.mask(ids, None, starts, None, None, select=0)[0]


@pytest.mark.parametrize("index", range(len(fh.cases())), ids=fh.CASE_IDS)
def test_token_level_matches_plain_python(tok, index):
    c = fh.cases()[index]
    seqs, labels, info, counts = fh.expected(index)
    ids, starts = fh.flat_arrays(index)
    ctx = tok._device()
    doc_arg = starts if starts is not None else 0  # (0: a NULL doc_off with one document)
    got = ctx.fim_to_host(ids, None, doc_arg, 1, None, **fh.native_kwargs(c))
    assert as_lists(got) == (seqs, labels, info)
    st = ctx.fim_stats()
    assert {k: st[k] for k in COUNTERS} == counts
    if len(ids) and index % 3 == 0:  # the ids in device memory, the starts on the host
        d_ids = device_copy(ctx, ids, starts)
        again = ctx.fim_to_host(d_ids, len(ids), doc_arg, 1, None, **fh.native_kwargs(c))
        assert all(np.array_equal(a, b) for a, b in zip(again, got))
        assert np.array_equal(ctx.d2h(d_ids, 4 * len(ids), np.uint32), ids)  # the inputs are left alone


@pytest.mark.parametrize("index", range(len(fh.cases())), ids=fh.CASE_IDS)
def test_pieces_match_plain_python(tok, index):
    c = fh.cases()[index]
    lens3, cuts, (seqs, labels, info, counts) = fh.pieces(index)
    ids, _ = fh.flat_arrays(index)
    starts = mh.starts(lens3)
    ctx = tok._device()
    got = ctx.fim_to_host(ids, None, starts, None, cuts, pieces=True, **fh.native_kwargs(c))
    assert as_lists(got) == (seqs, labels, info)
    st = ctx.fim_stats()
    assert {k: st[k] for k in COUNTERS} == counts
    if len(ids) and index % 3 == 1:  # ids, starts and cuts in device memory: what yabpe_encode and yabpe_fim_cuts hand over
        pad = np.zeros(len(ids) % 2, np.uint32)  # (the u64 tables behind the ids start on 8 bytes)
        blob = np.concatenate((ids, pad, starts.view(np.uint32), cuts.ravel().view(np.uint32)))
        d_ids = device_copy(ctx, blob, None)
        d_starts = d_ids + 4 * (len(ids) + len(pad))
        d_cuts = d_starts + 8 * len(starts)
        again = ctx.fim_to_host(d_ids, len(ids), d_starts, len(starts), d_cuts, pieces=True, **fh.native_kwargs(c))
        assert all(np.array_equal(a, b) for a, b in zip(again, got))


def test_the_python_twin_takes_the_users_numbers(tok):
    lens = [3, 0, 400, 1, 1, 90, 0]
    ids_b = mh.synth_batch(lens, seed=3)[0]
    ids = mh.flat(ids_b, np.uint32)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    for kw in ({}, {"fim_rate": 0.9, "spm_rate": 0.3, "seed": 9, "first_doc": 5, "eot": "<|endoftext|>"}, {"max_length": 50, "loss": "middle", "eot": 7},
               {"fim_rate": 0}, {"fim_rate": 1, "spm_rate": 1, "max_length": 4}):
        kw = {"pre": "[MASK]", "suf": "[PAD]", "mid": fh.MID, **kw}
        assert as_lists(tok.fim_array(ids, off, **kw)) == tok.fim_tokens(ids_b, **kw), kw


def test_results_outlive_later_calls_and_a_second_call_replaces_them(tok):
    from tests import span_helpers as sh

    lens = [5, 0, 300, 2]
    ids_b = mh.synth_batch(lens, seed=5)[0]
    ids, starts = mh.flat(ids_b, np.uint32), mh.starts(lens)
    ctx = tok._device()
    kw = {"seed": 1, "fim": 1 << 31, "spm": 1 << 31, "pre_id": fh.PRE, "suf_id": fh.SUF, "mid_id": fh.MID, "eot_id": fh.EOT}
    di, dl, do, dn, n_out, nd = ctx.fim(ids, None, starts, None, None, **kw)
    dpo, dcu, _ = ctx.fim_cuts("naïve text".encode("utf-8"), None, None, seed=1, fim=1 << 32, spm=0)

    def read():
        return (ctx.d2h(di, 4 * n_out, np.uint32), ctx.d2h(dl, 4 * n_out, np.uint32), ctx.d2h(do, 8 * (nd + 1), np.uint64), ctx.d2h(dn, 16 * nd, np.uint32),
                ctx.d2h(dpo, 24, np.uint64), ctx.d2h(dcu, 24, np.uint64))

    first = read()
    rows, _lengths = ctx.layout_pad_to_host(di, n_out, do, nd, row_len=16, pad_id=0)  # a layout call over the results ...
    tok.encode_array(mh.word_docs()[:20])
    tok.encode_array_padded(mh.word_docs()[:20], 16)
    tok.mask_array(ids, np.concatenate(([0], np.cumsum(lens))), mask_id=5000, n_random=7)
    tok.corrupt_spans_array(ids, np.concatenate(([0], np.cumsum(lens))), sentinels=sh.sentinels(100))
    assert all(np.array_equal(a, b) for a, b in zip(first, read()))  # ... and later calls leave them valid
    tok_py = type(tok)()
    py = {"pre": fh.PRE, "suf": fh.SUF, "mid": fh.MID, "eot": fh.EOT}
    exp = tok_py.fim_tokens(ids_b, seed=1, **py)
    assert fh.ragged(first[0], first[2]) == exp[0] and fh.ragged(first[1].view(np.int32), first[2]) == exp[1]
    assert rows.tolist() == tok_py._padded_rows(exp[0], 16, 0, 0, None, None, "right", "right")[0]
    ctx.fim(ids, None, starts, None, None, **{**kw, "seed": 2})  # a second yabpe_fim replaces its own results, not the cuts
    assert np.array_equal(ctx.d2h(dpo, 24, np.uint64), first[4]) and np.array_equal(ctx.d2h(dcu, 24, np.uint64), first[5])
    got = ctx.fim_to_host(ids, None, starts, None, None, **{**kw, "seed": 2})
    assert as_lists(got) == tok_py.fim_tokens(ids_b, seed=2, **py)
    ctx.fim_free()
    ctx.fim_free()
    got = ctx.fim_to_host(ids, None, starts, None, None, **{**kw, "seed": 2})  # and after a free
    assert as_lists(got) == tok_py.fim_tokens(ids_b, seed=2, **py)


def test_refused_arguments(tok):
    from yet_another_bpe import _native

    ids = np.arange(10, dtype=np.uint32)
    ctx = tok._device()
    ok = {"fim": 1 << 31, "spm": 1 << 31, "pre_id": fh.PRE, "suf_id": fh.SUF, "mid_id": fh.MID}
    good = ctx.fim_to_host(ids, None, [0, 4], None, None, **ok)
    stats = ctx.fim_stats()
    three, cuts3 = [0, 4, 6], np.zeros(3, np.uint64)
    cases = [({"fim": (1 << 32) + 1}, [0, 4], None), ({"spm": (1 << 32) + 1}, [0, 4], None), ({"max_len": 1}, [0, 4], None), ({"max_len": 3}, [0, 4], None),
             ({"max_len": 4, "eot_id": 5}, [0, 4], None), ({"flags": 8}, [0, 4], None), ({"pieces": True}, [0, 4], np.zeros(6, np.uint64)),
             ({"pieces": True}, three, None), ({}, three, cuts3), ({}, [1, 4], None), ({}, [0, 11], None), ({}, [0, 5, 4], None)]
    for bad, starts, cuts in cases:
        with pytest.raises(_native.YabpeError) as e:
            ctx.fim(ids, None, np.asarray(starts, np.uint64), None, cuts, **{**ok, **bad})
        assert e.value.code == E_INVALID, (bad, starts)
        assert ctx.fim_stats() == stats  # a refused call has changed nothing
    with pytest.raises(_native.YabpeError) as e:  # a NULL doc_off with two documents
        ctx.fim(ids, None, 0, 2, None, **ok)
    assert e.value.code == E_INVALID
    for n_ids in ((1 << 32), (1 << 36) + 1):  # a document of 2^32 ids; more than 2^36 slots: refused before anything is read or allocated
        with pytest.raises(_native.YabpeError) as e:
            ctx.fim(ids.ctypes.data, n_ids, 0, 1, None, **ok)
        assert e.value.code == E_CAPACITY and ctx.fim_stats() == stats
    with pytest.raises(_native.YabpeError) as e:  # the text calls refuse the same rule
        ctx.fim_cuts(b"abc", None, None, fim=(1 << 32) + 1)
    assert e.value.code == E_INVALID
    with pytest.raises(_native.YabpeError) as e:
        ctx.fim_cuts(b"abc", None, [0, 4], fim=1)
    assert e.value.code == E_INVALID and ctx.fim_stats() == stats
    # no result came back: the C call leaves every output zero
    f = _native.Fim(0, 0, (1 << 32) + 1, 0, 1, 2, 3, 0, 0, 0, 0)
    outs = [ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_void_p(1), ctypes.c_uint64(1)]
    rc = _native.lib().yabpe_fim(ctx._h, ctypes.c_void_p(ids.ctypes.data), 10, None, 1, None, ctypes.byref(f), *[ctypes.byref(o) for o in outs])
    assert rc == E_INVALID and not any(o.value for o in outs)
    assert len(ctx.fim_to_host(ids, None, three, None, cuts3, pieces=True, **ok)[2]) == 2
    again = ctx.fim_to_host(ids, None, [0, 4], None, None, **ok)
    assert all(np.array_equal(a, b) for a, b in zip(good, again))
    for bad in ({"fim_rate": 1.5}, {"max_length": 3}, {"max_length": 4, "eot": 7}, {"loss": "x"}, {"pre": "nope"}, {"seed": -1}, {"cuts": np.zeros((2, 3), np.uint64)}):
        with pytest.raises(ValueError):
            tok.fim_array(ids, [0, 10], **{"pre": fh.PRE, "suf": fh.SUF, "mid": fh.MID, **bad})
    with pytest.raises(ValueError):
        tok.fim_array(ids, [0, 4, 9], pre=fh.PRE, suf=fh.SUF, mid=fh.MID)  # doc_off must end at len(ids)
