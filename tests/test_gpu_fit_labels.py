"""GPU: yabpe_layout_fit_labels array for array against the plain-Python BBPETokenizer.fit_labelled, over the three label forms
and the smallest shapes that reach each branch of the write pass (a tile is FITL_TILE slots, a stage FITL_STAGE records); then
device-pointer inputs whose results outlive a later yabpe_encode, conversations from text, and refused arguments."""
from __future__ import annotations

import numpy as np
import pytest

from tests import chat_helpers as ch
from yet_another_bpe import _native

pytestmark = pytest.mark.gpu
IGN = -100
T, S = _native.FITL_TILE, _native.FITL_STAGE
rng = np.random.default_rng(7)
SHAPES = {  # name -> (C, sequence lengths)
    "edges": (8, [0, 1, 2, 7, 8, 11]),
    "odd-row-three-tiles": (37, rng.integers(1, 41, 3 * T // 21).tolist()),  # rows and sequences straddle the tile edges
    "stage-rounds": (600, [1] * (2 * S + 90) + [5, 3] + [1] * 100),          # row 0: 594 records inside tile 0
    "alignments": (16, [8, 9, 10, 11, 12, 5, 6, 7]),                         # source starts 0, 0, 1, 3, 2, 2, 3, 1 modulo 4
    "all-ignore": (12, [5, 12, 3, 7, 1]),
    "none": (8, []),
    "only-empty": (8, [0, 0, 0]),
}
FORMS = {"aligned": ("aligned", False), "aligned-mask-first": ("aligned", True), "shifted": ("shifted", True)}


@pytest.fixture(scope="module")
def tok():
    return ch.tokenizer()


def ragged(name):
    """-> (ids per sequence, labels per sequence): labels are 5000 + the id, `ignore` at every fifth id (all-ignore: everywhere)"""
    _C, lens = SHAPES[name]
    at = np.concatenate(([0], np.cumsum(lens, dtype=np.int64))).tolist()
    ids = [list(range(a + 1, b + 1)) for a, b in zip(at[:-1], at[1:])]
    return ids, [[IGN if name == "all-ignore" or t % 5 == 0 else 5000 + t for t in seq] for seq in ids]


def flat(ids, labels):
    off = np.concatenate(([0], np.cumsum([len(s) for s in ids], dtype=np.int64))).astype(np.uint64)
    cat = lambda rows, dt: np.asarray([t for r in rows for t in r], dtype=dt)  # noqa: E731
    return cat(ids, np.uint32), cat(labels, np.int32), off


def as_lists(got, C):
    assert got["labels"].dtype == np.int32 and all(got[k].shape[1:] == (C,) for k in ("ids", "labels", "seq", "pos"))
    out = {k: v.tolist() for k, v in got.items()}
    out["placed"] = [tuple(r) for r in out["placed"]]
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_matches_plain_python(tok, shape, form):
    C, lens = SHAPES[shape]
    ids, labels = ragged(shape)
    kw = {"pad_id": 9, "mask_first": FORMS[form][1]}
    exp = tok.fit_labelled(ids, labels, C, labels=FORMS[form][0], **kw)
    got = tok.fit_labelled_array(*flat(ids, labels), C, labels_form=FORMS[form][0], **kw)
    assert as_lists(got, C) == exp
    st = tok._device().layout_stats()
    kept = [min(n, C) for n in lens]
    assert (st["n_docs"], st["n_rows"], st["row_len"]) == (len(lens), len(exp["ids"]), C)
    assert (st["n_truncated_docs"], st["n_ids_dropped"]) == (sum(n > C for n in lens), sum(lens) - sum(kept))
    assert st["n_pad_slots"] == len(exp["ids"]) * C - sum(kept)
    if shape == "stage-rounds":  # the shape is what it claims to be
        assert exp["row_first"][1] > 2 * S and C < T
    if shape == "odd-row-three-tiles":
        assert 2 * T < len(exp["ids"]) * C <= 4 * T and T % C


def test_device_inputs_and_results_that_outlive_a_later_encode(tok):
    C = 16
    ids, labels, off = flat(*ragged("alignments"))
    ctx = tok._device()
    first = ctx.layout_fit_labels_to_host(ids, labels, None, off[:-1], None, row_len=C, pad_id=9, shifted=True)
    blob = np.concatenate((ids, labels.view(np.uint32), off[:-1].view(np.uint32)))  # (2 * 68 words in front: the starts are 8-byte aligned)
    d_ids = ctx.mask(blob, None, None, None, None, select=0)[0]  # (a mask that selects nothing copies the blob to the device)
    w = ctx.layout_fit_labels(d_ids, d_ids + 4 * len(ids), len(ids), d_ids + 8 * len(ids), len(off) - 1, row_len=C, pad_id=9, shifted=True)
    nr, npl = w["n_rows"], w["n_placed"]
    read = lambda: {**{k: ctx.d2h(w[k], 4 * nr * C, np.uint32).reshape(nr, C) for k in ("ids", "labels", "seq", "pos")},  # noqa: E731
                    **{k: ctx.d2h(w[k], 4 * nr, np.uint32) for k in ("used", "labelled")},
                    "placed": ctx.d2h(w["placed"], 12 * npl, np.uint32).reshape(npl, 3), "row_first": ctx.d2h(w["row_first"], 4 * (nr + 1), np.uint32)}
    same = lambda: all(np.array_equal(first[k].view(np.uint32), v) for k, v in read().items())  # noqa: E731
    assert same()
    tok.encode_array(["some text", "more"])
    ctx.mask(blob, None, None, None, None, select=0)
    assert same()  # later calls leave the results valid
    ctx.layout_free()
    ctx.layout_free()


CONVS = [[("system", "You are terse."), ("user", "Hello there, General Kenobi!"), ("assistant", "Hello."), ("user", "12345 naïve<|im_end|>"),
          ("assistant", "")], [], [{"role": "assistant", "content": "It's the end."}], [("user", "")], [("user", "Hi"), ("assistant", "Hello there.")]]


@pytest.mark.parametrize("kw", [{}, {"labels": "aligned", "pad_id": 3}, {"labels": "aligned", "mask_first": False, "truncation": "right"}])
def test_conversations_from_text_match_plain_python(tok, kw):
    exp = tok.encode_batch_chat_fit(CONVS, 40, **kw)
    got = tok.encode_array_chat_fit(CONVS, 40, **kw)
    info = [tuple(r) for r in got.pop("info").tolist()]
    assert info == exp.pop("info") and as_lists(got, 40) == exp
    assert kw.get("truncation") == "right" or info[0][1] > info[0][0]  # drop_oldest cut whole turns of the first conversation
    assert max(n for _s, _c, n in exp["placed"]) <= 40 and len(exp["placed"]) == sum(i[2] > 0 for i in info)
    assert tok.encode_array_chat_fit([], 40)["row_first"].tolist() == [0]


def test_refused_arguments_leave_the_previous_results_valid(tok):
    ids, labels, off = flat(*ragged("edges"))
    ctx = tok._device()
    w = ctx.layout_fit_labels(ids, labels, None, off[:-1], None, row_len=8, pad_id=9)
    good, stats = ctx.d2h(w["labels"], 4 * w["n_rows"] * 8, np.uint32), ctx.layout_stats()
    late, shifted = off[:-1].copy(), off[:-1] + np.uint64(1)
    late[2] = 99
    for bad, starts in (({"flags": 0x4}, off[:-1]), ({"row_len": 0}, off[:-1]), ({"row_len": 1 << 24}, off[:-1]), ({}, late), ({}, shifted)):
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_fit_labels(ids, labels, None, starts, None, **{"row_len": 8, **bad})
        assert e.value.code == -1, bad
        assert ctx.layout_stats() == stats and np.array_equal(ctx.d2h(w["labels"], 4 * w["n_rows"] * 8, np.uint32), good)  # nothing was freed
    for bad in ({"off": off[:-1]}, {"labels": labels[:-1]}, {"seq_len": 0}, {"labels_form": "x"}):
        a = {"ids": ids, "labels": labels, "off": off, "seq_len": 8, **bad}
        with pytest.raises(ValueError):
            tok.fit_labelled_array(a.pop("ids"), a.pop("labels"), a.pop("off"), a.pop("seq_len"), **a)
