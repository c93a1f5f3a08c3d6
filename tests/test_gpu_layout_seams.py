"""GPU: the seams between the four layout calls (yabpe_layout_pad / _pack / _windows / _pairs), which share one write kernel for
row records and one driver skeleton.  Synthetic ids through _native.Context:
  * yabpe_layout_pairs in windows mode with every first side empty and no separator is yabpe_layout_windows on the second sides:
    both are held against each other and against numpy (tests/window_helpers.py), at the row lengths, document lengths and
    totals where the shared writer takes another path;
  * every argument refusal and the reachable capacity refusals of the four calls, word for word;
  * what a refused call leaves behind: the previous call's buffers and stats after an argument refusal, empty stats after a
    capacity refusal found behind the count pass, and the stats of a call without pairs."""
from __future__ import annotations

import numpy as np
import pytest

from tests import layout_helpers as lh
from tests import pair_helpers as ph
from tests import window_helpers as wh

pytestmark = pytest.mark.gpu
E_INVALID, E_CAPACITY = -1, -4
BOS, EOS = ph.BOS, ph.EOS


@pytest.fixture(scope="module")
def ctx():
    from yet_another_bpe import _native

    with _native.Context() as c:
        yield c


def same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, k, g.dtype, g.shape, e.shape)
        assert np.array_equal(g, e), (what, k, np.argwhere(g != e)[:5].tolist())


def np_types(lengths, L, bos, pad_left):
    """1 on the content and EOS slots of window rows of `lengths` kept slots: every kept slot but BOS"""
    kept = lengths.astype(np.int64)
    p = np.arange(L, dtype=np.int64)[None, :] - ((L - kept)[:, None] if pad_left else 0)
    return ((p >= (bos is not None)) & (p < kept[:, None])).astype(np.uint8)


def windows_both_ways(ctx, lens, L, stride, bos, eos, pl, spans):
    """layout_windows on `lens`, layout_pairs in windows mode on [0, lens[0], 0, lens[1], ...], numpy -> slots in the output"""
    ids, starts = wh.synth(lens)
    sp = wh.synth_spans(len(ids)) if spans else None
    what = (lens if len(lens) < 9 else len(lens), L, stride, bos, eos, pl, spans)
    exp = wh.np_windows(ids, lens, L, stride, wh.PAD, bos, eos, pl, sp)
    win = ctx.layout_windows_to_host(ids, doc_starts=starts, spans=sp, row_len=L, stride=stride, pad_id=wh.PAD, bos_id=bos, eos_id=eos, pad_left=pl)
    same(win, exp, ("windows", what))
    pair_starts = np.repeat(starts, 2)  # an empty first side in front of every document
    got = ctx.layout_pairs_to_host(ids, doc_starts=pair_starts, spans=sp, row_len=L, mode="windows", stride=stride, sep_id=None, n_sep=0,
                                   pad_id=wh.PAD, bos_id=bos, eos_id=eos, pad_left=pl)
    rows, types, row_pair, row_start, first_len, second_len = got[:6]
    n_added = np.uint32((bos is not None) + (eos is not None))
    same((rows, row_pair, row_start, second_len + n_added) + got[6:], win, ("pairs against windows", what))
    assert not first_len.any(), what
    assert types.dtype == np.uint8 and np.array_equal(types, np_types(exp[3], L, bos, pl)), what
    return rows.size


# (row_len, stride, bos, eos): a row boundary inside a thread's four slots (1, 2, 3, 5), several rows per 16-byte store (1, 2, 3),
# a row of two stores (8); every framing; step 1 and more
SHAPES = ((1, 0, None, None), (2, 0, BOS, None), (3, 1, None, EOS), (5, 1, BOS, EOS), (5, 4, None, None), (8, 2, BOS, EOS))


def test_pairs_with_empty_first_sides_are_windows(ctx):
    tails = set()
    for L, stride, bos, eos in SHAPES:
        C = L - (bos is not None) - (eos is not None)
        for extra in range(4 if L % 2 else 2):  # (a further empty document is a further row: the tail of the last store moves)
            lens = [0, C, C + 1, 301] + [0] * extra  # one row, one full row, two rows, many
            for pl in (False, True):
                for spans in (False, True):
                    tails.add(windows_both_ways(ctx, lens, L, stride, bos, eos, pl, spans) % 4)
    assert tails == {0, 1, 2, 3}  # the tail stores of ids and of type bytes: 1, 2 and 3 slots past the last whole vector


def test_the_second_workgroup_of_the_write_and_of_the_rows_kernel(ctx):
    for pl in (False, True):
        for spans in (False, True):
            n_slots = windows_both_ways(ctx, [3000, 0, 3], 5, 1, BOS, None, pl, spans)
            assert n_slots > 4096 and n_slots // 5 > 256  # (a write workgroup owns 4,096 slots, a rows workgroup 256 rows)


# ---- refusals
LENS = [3, 4, 2, 5]
FIRST_NOT_0 = "doc_off must hold n_docs >= 1 starts, the first one 0"
NOT_ASCENDING = "document starts must ascend inside the ids"
BAD_STARTS = (([1, 3], FIRST_NOT_0), ([0, 5, 4, 9], NOT_ASCENDING), ([0, 15], NOT_ASCENDING))
TRUNC_LEFT, DROP_LAST, UNKNOWN = 0x04, 0x10, 0x20  # LAYOUT_TRUNC_LEFT, LAYOUT_DROP_LAST, no flag


def refusals():
    """call -> [(keyword arguments, error code, message)]: the argument refusals of the call, found before anything is freed"""
    return {
        "pad": [
            ({"row_len": 1, "bos_id": 1, "eos_id": 2}, E_INVALID, "row_len 1 cannot hold BOS and EOS"),
            ({"row_len": 4, "flags": DROP_LAST}, E_INVALID, "layout flags 0x10 do not belong to this call (it takes 0xf)"),
            ({"row_len": 4, "flags": UNKNOWN}, E_INVALID, "unknown layout flags 0x20"),
            ({"row_len": 1 << 31, "doc_starts": np.zeros(128, np.uint64)}, E_CAPACITY, "128 rows of 2147483648 slots: at most 2^36 slots in one call"),
        ],
        "pack": [
            ({"row_len": 0}, E_INVALID, "row_len is 0: a packed row holds at least one slot"),
            ({"row_len": 4, "flags": TRUNC_LEFT}, E_INVALID, "layout flags 0x4 do not belong to this call (it takes 0x13)"),
            ({"row_len": 4, "flags": UNKNOWN}, E_INVALID, "unknown layout flags 0x20"),
        ],
        "windows": [
            ({"row_len": 1, "bos_id": 1}, E_INVALID, "row_len 1 leaves no slot for content beside BOS and EOS"),
            ({"row_len": 4, "stride": 4}, E_INVALID, "stride 4: consecutive rows of 4 content slots must advance by at least one"),
            ({"row_len": 4, "flags": TRUNC_LEFT}, E_INVALID, "layout flags 0x4 do not belong to this call (it takes 0xb)"),
            ({"row_len": 4, "flags": DROP_LAST}, E_INVALID, "layout flags 0x10 do not belong to this call (it takes 0xb)"),
            ({"row_len": 4, "flags": UNKNOWN}, E_INVALID, "unknown layout flags 0x20"),
        ],
        "pairs": [
            ({"row_len": 3, "bos_id": 1, "eos_id": 2, "sep_id": 3}, E_INVALID, "row_len 3 leaves no slot for content beside BOS, EOS and 1 separators"),
            ({"row_len": 4, "mode": "windows", "stride": 4}, E_INVALID,
             "stride 4: a row of 4 content slots must keep one more than the stride for the second side"),
            ({"row_len": 4, "flags": TRUNC_LEFT}, E_INVALID, "layout flags 0x4 do not belong to this call (it takes 0xb)"),
            ({"row_len": 4, "flags": DROP_LAST}, E_INVALID, "layout flags 0x10 do not belong to this call (it takes 0xb)"),
            ({"row_len": 4, "flags": UNKNOWN}, E_INVALID, "layout flags 0x20 do not belong to this call (it takes 0xb)"),  # (this call's own check comes first)
            ({"row_len": 4, "doc_starts": np.asarray([0, 3, 7], np.uint64)}, E_INVALID,
             "3 documents: documents 2p and 2p + 1 are pair p, so their number is even"),
            ({"row_len": 9, "sep_id": 3, "n_sep": 3}, E_INVALID, "n_sep 3: at most 2 separators between the two sides"),
            ({"row_len": 9, "mode": 4}, E_INVALID, "unknown pairs mode 4"),
            ({"row_len": 9, "stride": 1}, E_INVALID, "stride 1: only windows mode takes a stride"),
            ({"row_len": 1 << 31, "doc_starts": np.zeros(128, np.uint64)}, E_CAPACITY, "64 pairs in rows of 2147483648 slots: at most 2^36 slots in one call"),
        ],
    }


def refused(ctx, call, kw, code, text):
    from yet_another_bpe import _native

    ids, starts = lh.synth(LENS)
    kw = {"doc_starts": starts, **kw}
    with pytest.raises(_native.YabpeError) as e:
        getattr(ctx, "layout_" + call)(ids, **kw)
    assert e.value.code == code and str(e.value) == f"yabpe error {code}: {text}", (call, kw, str(e.value))


def good(ctx, call):
    """a good call of each kind gives what numpy gives"""
    ids, starts = lh.synth(LENS)
    sp = wh.synth_spans(len(ids))
    if call == "pad":
        same(ctx.layout_pad_to_host(ids, doc_starts=starts, row_len=4, pad_id=lh.PAD, eos_id=EOS), lh.np_pad(ids, LENS, 4, lh.PAD, None, EOS, False, False), call)
    elif call == "pack":
        same(ctx.layout_pack_to_host(ids, doc_starts=starts, row_len=4, pad_id=lh.PAD, eos_id=EOS), lh.np_pack(ids, LENS, 4, lh.PAD, None, EOS, False), call)
    elif call == "windows":
        same(ctx.layout_windows_to_host(ids, doc_starts=starts, spans=sp, row_len=4, stride=1, pad_id=wh.PAD, bos_id=BOS),
             wh.np_windows(ids, LENS, 4, 1, wh.PAD, BOS, None, False, sp), call)
    else:
        same(ctx.layout_pairs_to_host(ids, doc_starts=starts, spans=sp, row_len=6, mode="windows", stride=1, sep_id=ph.SEP, pad_id=ph.PAD, bos_id=BOS),
             ph.np_pairs(ids, LENS, 6, "windows", 1, ph.PAD, BOS, None, ph.SEP, 1, False, sp), call)


def test_refusals_word_for_word(ctx):
    for call, cases in refusals().items():
        for kw, code, text in cases:
            refused(ctx, call, kw, code, text)
            good(ctx, call)
        for bad_starts, text in BAD_STARTS:
            refused(ctx, call, {"row_len": 6, "doc_starts": np.asarray(bad_starts, np.uint64)}, E_INVALID, text)
            good(ctx, call)


def over_2_36(ctx, call):
    """2^20 + 1 rows of 2^16 slots, known from the scan's total: refused behind the count pass, which has released the last results"""
    from yet_another_bpe import _native

    ids = np.zeros((1 << 20) + (1 << 16), np.uint32)
    kw = {"doc_starts": np.zeros(2, np.uint64), "mode": "windows"} if call == "pairs" else {}
    with pytest.raises(_native.YabpeError) as e:
        getattr(ctx, "layout_" + call)(ids, row_len=1 << 16, stride=(1 << 16) - 1, **kw)
    assert e.value.code == E_CAPACITY and str(e.value) == "yabpe error -4: 1048577 rows of 65536 slots: at most 2^36 slots in one call", str(e.value)


def test_what_a_refused_call_leaves_behind(ctx):
    lens = [5, 0, 9]
    ids, starts = wh.synth(lens)
    sp = wh.synth_spans(len(ids))
    exp = wh.np_windows(ids, lens, 4, 1, wh.PAD, None, EOS, False, sp)
    dr, dd, ds, dl, dsp, nr = ctx.layout_windows(ids, doc_starts=starts, spans=sp, row_len=4, stride=1, pad_id=wh.PAD, eos_id=EOS)
    stats = ctx.layout_stats()
    assert nr == len(exp[0]) == stats["n_rows"]

    def call_a_is_still_there(what):
        got = (ctx.d2h(dr, 16 * nr, np.uint32).reshape(nr, 4),) + tuple(ctx.d2h(p, 4 * nr, np.uint32) for p in (dd, ds, dl))
        same(got + (ctx.d2h(dsp, 64 * nr, np.uint64).reshape(nr, 4, 2),), exp, what)
        assert ctx.layout_stats() == stats, what

    for call, cases in refusals().items():
        for kw, code, text in cases:
            refused(ctx, call, kw, code, text)
            call_a_is_still_there((call, kw))
        for bad_starts, text in BAD_STARTS:
            refused(ctx, call, {"row_len": 6, "doc_starts": np.asarray(bad_starts, np.uint64)}, E_INVALID, text)
            call_a_is_still_there((call, bad_starts))
    for call in ("windows", "pairs"):
        good(ctx, call)
        assert ctx.layout_stats()["n_rows"] > 0
        over_2_36(ctx, call)
        st = ctx.layout_stats()
        assert st["n_rows"] == 0 and st["row_len"] == 0 and st["n_docs"] == (2 if call == "pairs" else 1), st
        good(ctx, call)
    # no pairs: the last results go, the stats are those of an empty batch of the row length asked for
    for kw in ({}, {"mode": "windows", "stride": 2}):
        out = ctx.layout_pairs_to_host(np.zeros(0, np.uint32), doc_starts=np.zeros(0, np.uint64), spans=wh.synth_spans(0), row_len=7, bos_id=BOS, **kw)
        assert [a.shape for a in out] == [(0, 7), (0, 7), (0,), (0,), (0,), (0,), (0, 7, 2)]
        st = ctx.layout_stats()
        assert {k: v for k, v in st.items() if v} == {"row_len": 7}, st
        good(ctx, "pairs")
