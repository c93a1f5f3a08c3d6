"""GPU: text pairs (yabpe_layout_pairs).  Synthetic ids through Context.layout_pairs_to_host against numpy
(tests/pair_helpers.py, held against the plain-Python contract by tests/test_pairs_model.py) over the grid of row lengths,
separators, framing ids, sides and modes, with and without spans, and the pair lengths that take the kernels' other paths; the
tokenizer's encode_array_pairs against encode_batch_pairs; device inputs, errors, stats and results that outlive the next
encode."""
from __future__ import annotations

import numpy as np
import pytest

from tests import pair_helpers as ph
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
IDENT = {bytes([i]): i for i in range(256)}
E_INVALID, E_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from yet_another_bpe import _native

    with _native.Context() as c:
        yield c


def same(got, exp, what):
    assert len(got) == len(exp), what
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, g.dtype, g.shape, e.shape)
        assert np.array_equal(g, e), (what, np.argwhere(g != e)[:5].tolist())


def both(ctx, lens, L, mode, stride, bos, eos, sep, n_sep, pl, spans=False, pad=ph.PAD, ids=None):
    """-> what the device gives, what numpy gives"""
    if ids is None:
        ids, starts = ph.synth(lens)
    else:
        starts = ph.synth(lens)[1]
    sp = ph.synth_spans(len(ids)) if spans else None
    got = ctx.layout_pairs_to_host(ids, doc_starts=starts, spans=sp, row_len=L, mode=mode, stride=stride, sep_id=sep, n_sep=n_sep, pad_id=pad,
                                   bos_id=bos, eos_id=eos, pad_left=pl)
    return got, ph.np_pairs(ids, lens, L, mode, stride, pad, bos, eos, sep, n_sep, pl, sp)


def test_pairs_grid(ctx):
    n_cases = 0
    for L, mode, stride, bos, eos, sep, n_sep, pl in ph.pair_cases():
        lens = ph.pair_lengths(L - ph.n_added_of(bos, eos, sep, n_sep), mode, stride)
        got, exp = both(ctx, lens, L, mode, stride, bos, eos, sep, n_sep, pl, True)
        same(got, exp, (L, mode, stride, bos, eos, sep, n_sep, pl, "spans"))
        ids, starts = ph.synth(lens)
        got = ctx.layout_pairs_to_host(ids, doc_starts=starts, row_len=L, mode=mode, stride=stride, sep_id=sep, n_sep=n_sep, pad_id=ph.PAD,
                                       bos_id=bos, eos_id=eos, pad_left=pl)
        same(got, exp[:6], (L, mode, stride, bos, eos, sep, n_sep, pl))
        n_cases += 1
    assert n_cases > 400


def test_other_paths(ctx):
    for spans in (False, True):
        # step 1: many 4,096-slot write pieces from one pair
        got, exp = both(ctx, [0, 20000], 8, "windows", 7, None, None, None, 0, False, spans)
        same(got, exp, "one pair, step 1")
        assert got[0].shape == (20000 - 8 + 1, 8)
        same(*both(ctx, [5, 20000], 12, "windows", 3, 1, 2, 3, 2, True, spans), "one pair, the first side in every row")
        # more pairs than a count workgroup, more rows in a piece than a 2,048-offset stage
        for mode in ("longest_first", "windows"):
            got, exp = both(ctx, [1, 1] * 5000, 2, mode, 0, None, None, None, 0, False, spans)
            same(got, exp, ("5,000 pairs", mode))
            assert got[0].shape == (5000, 2) and np.array_equal(got[2], np.arange(5000)) and (got[1] == [0, 1]).all()
        for mode in ph.MODES:  # a row longer than a write piece
            same(*both(ctx, [3, 9000, 6000, 2, 0, 0], 5000, mode, 0, 1, 2, 3, 1, False, spans), ("row_len 5000", mode))
        same(*both(ctx, [7000, 4300], 4099, "windows", 4000, None, 2, 3, 2, True, spans), "row_len 4099, stride 4000")
        for mode in ph.MODES:
            got, exp = both(ctx, [0] * 6, 4, mode, 0, 1, None, 3, 1, True, spans)
            same(got, exp, ("only empty documents", mode))
            assert got[0].tolist() == [[ph.PAD, ph.PAD, 1, 3]] * 3 and not got[1].any()
        big = 0xFFFFFFFE  # ids next to the top of u32 come back unchanged
        for mode in ph.MODES:
            got, exp = both(ctx, [3, 0, 6, 2], 6, mode, 0, big, big, big, 1, True, spans, pad=big, ids=np.full(11, big, np.uint32))
            same(got, exp, ("0xFFFFFFFE", mode))
            assert (got[0] == big).all()
        for mode in ph.MODES:  # no pairs at all
            got = ctx.layout_pairs_to_host(np.zeros(0, np.uint32), doc_starts=np.zeros(0, np.uint64), spans=ph.synth_spans(0) if spans else None,
                                           row_len=5, mode=mode, sep_id=3)
            assert [g.shape for g in got] == [(0, 5), (0, 5), (0,), (0,), (0,), (0,)] + ([(0, 5, 2)] if spans else [])
            assert [g.dtype for g in got[:2]] == [np.uint32, np.uint8]
            st = ctx.layout_stats()
            assert (st["n_docs"], st["n_rows"], st["row_len"], st["n_pad_slots"]) == (0, 0, 5, 0)


def test_device_inputs(ctx):
    """Context.encode_spans' device pointers passed straight in give what the host copies of the same arrays give."""
    tok = BBPETokenizer(vocab={**IDENT, b"th": 256, b"he": 257}, merges=[(b"t", b"h"), (b"h", b"e")])
    docs = [b"the other thing", b"", b"he then", b"x" * 100, b"", b"", b"which", b"that other one there"]
    starts = np.cumsum([0] + [len(d) for d in docs[:-1]]).astype(np.uint64)
    ctx.encode_set_model(tok._vocab, tok._merges, [], 0)
    di, dd, ds, ni = ctx.encode_spans(b"".join(docs), doc_starts=starts)
    ids, off, spans = ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), ctx.d2h(ds, 16 * ni, np.uint64).reshape(-1, 2)
    assert [ids[off[d]:off[d + 1]].tolist() for d in range(len(docs))] == tok.encode_batch([d.decode() for d in docs])
    lens = np.diff(off.astype(np.int64))
    for kw in ({"row_len": 9, "bos_id": 7, "sep_id": 6, "n_sep": 2}, {"row_len": 12, "mode": "windows", "stride": 3, "eos_id": 8, "pad_left": True},
               {"row_len": 200, "mode": "only_second", "sep_id": 5}, {"row_len": 1, "mode": "only_first"}):
        dev = ctx.layout_pairs_to_host(di, ni, dd, len(docs), ds, pad_id=999, **kw)
        same(dev, ctx.layout_pairs_to_host(ids, doc_starts=off[:-1], spans=spans, pad_id=999, **kw), kw)
        same(dev, ph.np_pairs(ids, lens, kw["row_len"], kw.get("mode", "longest_first"), kw.get("stride", 0), 999, kw.get("bos_id"), kw.get("eos_id"),
                              kw.get("sep_id"), kw.get("n_sep", 1), kw.get("pad_left", False), spans), kw)
        same(ctx.layout_pairs_to_host(di, ni, dd, len(docs), pad_id=999, **kw), dev[:6], (kw, "without spans"))
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), ids)  # the layout calls left the encoder's results alone
    assert np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), off)
    assert np.array_equal(ctx.d2h(ds, 16 * ni, np.uint64).reshape(-1, 2), spans)


SPECIALS = ["<|endoftext|>", "<|x|>"]
# (precomposed and decomposed accents: a normaliser changes the second kind)
FIRSTS = ["who wrote the thing?", "", "\u00e9", "<|x|>the <|endoftext|> then", "the\u0301 caf\u00e9 \u4e2d\u6587 \U0001F600", "x" * 70, "he", ""]
SECONDS = ["the other one wrote it, then the other <|endoftext|> he", "", "", "th\u00e9 " * 30, "e\u0301\u00e9 the", "yz", "<|x|>" * 9, "then"]


def small_tok(normalizer=None):
    vocab = {**IDENT, b"th": 256, b"he": 257, b"the": 258, b" the": 259, b"\xc3\xa9": 260, b"<|endoftext|>": 300, b"[PAD]": 301}
    merges = [(b"t", b"h"), (b"h", b"e"), (b"th", b"e"), (b" ", b"the"), (b"\xc3", b"\xa9")]
    return BBPETokenizer(vocab=vocab, merges=merges, special_tokens=SPECIALS, normalizer=normalizer)  # ("<|x|>" has no id: a gap)


def tok_check(tok, firsts, seconds, what):
    cases = ({"max_length": 16, "sep_id": 400, "n_sep": 2, "bos_id": 401, "eos_id": 400},
             {"max_length": 9, "truncation": "only_first", "sep_id": 4_000_000_000, "padding_side": "left"},
             {"max_length": 12, "truncation": "only_second", "eos_id": 0, "pad_id": 3},
             {"max_length": 20, "truncation": "windows", "stride": 4, "bos_id": 401, "sep_id": 400, "eos_id": 400},
             {"max_length": 7, "truncation": "windows", "stride": 6, "padding_side": "left"}, {"max_length": 1})
    for kw in cases:
        for extra in ({}, {"offsets": "char"}, {"offsets": "byte"}):
            got = tok.encode_array_pairs(firsts, seconds, **kw, **extra)
            exp = tok.encode_batch_pairs(firsts, seconds, **kw, **extra)
            assert len(got) == len(exp) == (7 if extra else 6), (what, kw, extra)
            same(got, ph.as_arrays(exp, kw["max_length"]), (what, kw, extra))


def test_through_the_tokenizer():
    for normalizer in (None, "nfc"):
        tok = small_tok(normalizer)
        tok_check(tok, FIRSTS, SECONDS, normalizer)
        tok_check(tok, [], [], (normalizer, "no pairs"))
        tok_check(tok, ["", ""], ["", ""], (normalizer, "only empty texts"))
    # the two cross-checks of the contract, computed on the device
    tok = small_tok()
    texts = FIRSTS + SECONDS
    for L, bos, eos, side in ((1, None, None, "right"), (7, 401, None, "left"), (30, 401, 0, "right")):
        n_added = (bos is not None) + (eos is not None)
        kw = dict(pad_id=3, bos_id=bos, eos_id=eos, padding_side=side)
        rows, lengths = tok.encode_array_padded(texts, L, **kw)
        for mode in ph.MODES[:3]:
            got = tok.encode_array_pairs(texts, [""] * len(texts), L, truncation=mode, **kw)
            assert np.array_equal(got[0], rows) and np.array_equal(got[4] + n_added, lengths) and not got[5].any()
            assert int(got[1].sum()) == (len(texts) if eos is not None else 0)  # type 1 in the EOS slots alone
        for stride in sorted({0, L - n_added - 1}):
            for offsets in (None, "char", "byte"):
                exp = tok.encode_array_windows(texts, L, stride, offsets=offsets, **kw)
                got = tok.encode_array_pairs([""] * len(texts), texts, L, truncation="windows", stride=stride, offsets=offsets, **kw)
                same((got[0], got[2], got[3], got[5] + np.uint32(n_added)) + got[6:], exp, (L, stride, offsets))
                assert not got[4].any()


def test_errors_leave_the_context_usable(ctx):
    from yet_another_bpe import _native

    ids, starts = ph.synth([3, 4, 2, 5])
    bad = [
        ({"row_len": 0}, "row_len"),                                                   # row_len <= n_added
        ({"row_len": 1, "bos_id": 1}, "row_len"),
        ({"row_len": 3, "bos_id": 1, "eos_id": 2, "sep_id": 3}, "row_len"),
        ({"row_len": 4, "bos_id": 1, "eos_id": 2, "sep_id": 3, "n_sep": 2}, "row_len"),
        ({"row_len": 9, "sep_id": 3, "n_sep": 3}, "n_sep"),                            # n_sep > 2
        ({"row_len": 9, "sep_id": 3, "n_sep": 0xFFFFFFFF}, "n_sep"),
        ({"row_len": 9, "mode": 4}, "mode"),                                           # an unknown mode
        ({"row_len": 9, "mode": 0xFFFFFFFF}, "mode"),
        ({"row_len": 9, "stride": 1}, "stride"),                                       # a stride outside windows mode
        ({"row_len": 9, "mode": "only_first", "stride": 1}, "stride"),
        ({"row_len": 9, "mode": "only_second", "stride": 8}, "stride"),
        ({"row_len": 4, "mode": "windows", "stride": 4}, "stride"),                    # stride >= C
        ({"row_len": 6, "mode": "windows", "stride": 3, "eos_id": 2, "sep_id": 3, "n_sep": 2}, "stride"),
        ({"row_len": 4, "mode": "windows", "stride": 0xFFFFFFFF}, "stride"),
        ({"row_len": 4, "flags": _native.LAYOUT_TRUNC_LEFT}, "flags"),                 # flags of the other modes
        ({"row_len": 4, "flags": _native.LAYOUT_DROP_LAST}, "flags"),
        ({"row_len": 4, "flags": 0x20}, "flags"),                                      # an unknown flag
    ]
    for kw, word in bad:
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_pairs(ids, doc_starts=starts, **kw)
        assert e.value.code == E_INVALID and word in str(e.value), (kw, str(e.value))
    for odd in ([0, 3, 7], [0]):  # documents 2p and 2p + 1 are pair p
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_pairs(ids, doc_starts=np.asarray(odd, dtype=np.uint64), row_len=4)
        assert e.value.code == E_INVALID and "even" in str(e.value)
    for bad_starts in ([1, 3], [0, 5, 4, 9], [0, 15]):  # not from 0, not ascending, past the ids
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_pairs(ids, doc_starts=np.asarray(bad_starts, dtype=np.uint64), row_len=4)
        assert e.value.code == E_INVALID and "doc" in str(e.value)
    with pytest.raises(ValueError):  # not one span per id: refused by the binding
        ctx.layout_pairs(ids, doc_starts=starts, spans=ph.synth_spans(6), row_len=4)
    same(*both(ctx, [3, 4, 2, 5], 6, "longest_first", 0, 1, None, 3, 1, False, True), "a good call after the bad ones")
    # 64 pairs in rows of 2^31 slots: 2^37 slots, refused before anything is allocated
    for mode in ph.MODES:
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_pairs(np.zeros(0, np.uint32), doc_starts=np.zeros(128, np.uint64), row_len=1 << 31, mode=mode)
        assert e.value.code == E_CAPACITY and "2^36" in str(e.value)
    # ... and in windows mode also from the scan's total: 2^20 + 1 rows of 2^16 slots
    with pytest.raises(_native.YabpeError) as e:
        ctx.layout_pairs(np.zeros((1 << 20) + (1 << 16), np.uint32), doc_starts=np.zeros(2, np.uint64), row_len=1 << 16, mode="windows",
                         stride=(1 << 16) - 1)
    assert e.value.code == E_CAPACITY and "2^36" in str(e.value)
    same(*both(ctx, [3, 4, 2, 5], 6, "windows", 2, 1, None, 3, 1, False), "a good call after the refused ones")


def test_pairs_stats(ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, 1000).tolist()
    for (bos, eos, sep, n_sep), L, mode, stride in (((None, None, None, 0), 40, "longest_first", 0), ((1, None, 3, 1), 25, "only_first", 0),
                                                    ((1, 2, 3, 2), 30, "only_second", 0), ((None, 2, 3, 1), 64, "windows", 3),
                                                    ((1, 2, None, 0), 12, "windows", 9)):
        n_added = ph.n_added_of(bos, eos, sep, n_sep)
        for spans in (False, True):
            got, exp = both(ctx, lens, L, mode, stride, bos, eos, sep, n_sep, False, spans)
            same(got, exp, ("stats", L, mode))
            st = ctx.layout_stats()
            n_rows, n_cut, n_dropped, n_pad = ph.pair_stats(lens, exp, L, n_added, mode)
            assert n_rows == len(got[0]) and 0 < n_cut <= len(lens) // 2 and (n_dropped > 0) == (mode != "windows")
            assert n_pad == int((exp[0] == ph.PAD).sum())
            assert (st["n_ids"], st["n_docs"], st["n_rows"], st["row_len"]) == (sum(lens), len(lens), n_rows, L), st
            assert (st["n_truncated_docs"], st["n_ids_dropped"], st["n_pad_slots"]) == (n_cut, n_dropped, n_pad), st
            assert st["lengths_ms"] > 0 and st["write_ms"] > 0 and st["total_ms"] >= st["write_ms"], st


def test_results_outlive_the_next_encode(ctx):
    lens = [5, 9, 0, 3]
    ids, starts = ph.synth(lens)
    sp = ph.synth_spans(len(ids))
    *ptrs, nr = ctx.layout_pairs(ids, doc_starts=starts, spans=sp, row_len=8, mode="windows", stride=1, sep_id=3, pad_id=ph.PAD, eos_id=2)
    exp = ph.np_pairs(ids, lens, 8, "windows", 1, ph.PAD, None, 2, 3, 1, False, sp)
    ctx.encode_set_model(dict(IDENT), [], [], 0)
    ctx.encode_spans_to_host(b"other text " * 300)
    ctx.encode_free()
    assert nr == len(exp[0]) == 8 + 1  # C = 6: ka = 4, Cb = 2, step 1 over 9 ids; one row for the second pair
    got = (ctx.d2h(ptrs[0], 32 * nr, np.uint32).reshape(nr, 8), ctx.d2h(ptrs[1], 8 * nr, np.uint8).reshape(nr, 8)) + tuple(
        ctx.d2h(p, 4 * nr, np.uint32) for p in ptrs[2:6])
    same(got + (ctx.d2h(ptrs[6], 128 * nr, np.uint64).reshape(nr, 8, 2),), exp, "after the next encode")
    assert ctx.layout_pairs(ids, doc_starts=starts, row_len=8)[6] == 0  # no spans in: none out
    ctx.layout_free()
    ctx.layout_free()  # (twice is fine)
