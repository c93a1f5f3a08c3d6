"""GPU: overlapping windows (yabpe_layout_windows).  Synthetic ids through Context.layout_windows_to_host against numpy
(tests/window_helpers.py, held against the plain-Python contract by tests/test_windows_model.py) over the grid of row lengths,
framing ids, strides and sides, with and without spans, and the document lengths that take the kernels' other paths; the
tokenizer's encode_array_windows against encode_batch_windows; device inputs, errors, stats, results that outlive the next
encode, and the allocation trace of a fresh process."""
from __future__ import annotations

import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import encode_helpers, helpers
from tests import window_helpers as wh
from tests.test_gpu_pretok import SPECIALS
from tests.test_gpu_scratch_balance import ALLOC, FREE, mark
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


def both(ctx, lens, L, stride, bos, eos, pl, spans=False, pad=wh.PAD, ids=None):
    """-> what the device gives, what numpy gives"""
    if ids is None:
        ids, starts = wh.synth(lens)
    else:
        starts = wh.synth(lens)[1]
    sp = wh.synth_spans(len(ids)) if spans else None
    got = ctx.layout_windows_to_host(ids, doc_starts=starts, spans=sp, row_len=L, stride=stride, pad_id=pad, bos_id=bos, eos_id=eos, pad_left=pl)
    return got, wh.np_windows(ids, lens, L, stride, pad, bos, eos, pl, sp)


def test_windows_grid(ctx):
    for L, stride, bos, eos, pl in wh.win_cases():
        lens = wh.win_lengths(L, (bos is not None) + (eos is not None), stride)
        for spans in (False, True):
            same(*both(ctx, lens, L, stride, bos, eos, pl, spans), (L, stride, bos, eos, pl, spans))


def test_other_paths(ctx):
    for spans in (False, True):
        # step 1: one document over many 4,096-slot pieces
        got, exp = both(ctx, [20000], 8, 7, None, None, False, spans)
        same(got, exp, "one document, step 1")
        assert got[0].shape == (20000 - 8 + 1, 8)
        # more documents (and rows) in a piece than a 2,048-offset stage holds
        got, exp = both(ctx, [1] * 5000, 1, 0, None, None, False, spans)
        same(got, exp, "5,000 one-id documents")
        assert got[0].shape == (5000, 1) and np.array_equal(got[1], np.arange(5000))
        same(*both(ctx, [0, 0, 0], 4, 1, 1, None, True, spans), "only empty documents")
        got, exp = both(ctx, [0], 3, 0, 1, 2, False, spans)
        same(got, exp, "one empty document")
        assert got[0].tolist() == [[1, 2, wh.PAD]] and got[3].tolist() == [2]
        big = 0xFFFFFFFE  # ids next to the top of u32 come back unchanged
        got, exp = both(ctx, [3, 0, 6], 4, 1, big, big, True, spans, pad=big, ids=np.full(9, big, np.uint32))
        same(got, exp, "0xFFFFFFFE")
        assert (got[0] == big).all() and got[3].tolist() == [4, 4, 2, 4, 4, 4, 4, 4]
    ids = np.arange(10, dtype=np.uint32)  # one document, without document starts at all
    for spans in (None, wh.synth_spans(10)):
        got = ctx.layout_windows_to_host(ids, spans=spans, row_len=4, stride=2, pad_id=1, eos_id=2)
        same(got, wh.np_windows(ids, [10], 4, 2, 1, None, 2, False, spans), "n_docs = 1")
    for C, bos, eos in ((6, None, None), (6, 1, None), (6, 1, 2)):  # rows(n) at exactly n = C and n = C + 1
        L = C + (bos is not None) + (eos is not None)
        for stride in (0, 5):
            got, exp = both(ctx, [C, C + 1], L, stride, bos, eos, False, True)
            same(got, exp, (C, stride))
            assert got[1].tolist() == [0, 1, 1] and got[2].tolist() == [0, 0, C - stride] and got[3].tolist() == [L, L, L - C + stride + 1]


def test_device_inputs(ctx):
    """Context.encode_spans' device pointers passed straight in give what the host copies of the same arrays give."""
    tok = BBPETokenizer(vocab={**IDENT, b"th": 256, b"he": 257}, merges=[(b"t", b"h"), (b"h", b"e")])
    docs = [b"the other thing", b"", b"he then", b"x" * 100, b""]
    starts = np.cumsum([0] + [len(d) for d in docs[:-1]]).astype(np.uint64)
    ctx.encode_set_model(tok._vocab, tok._merges, [], 0)
    di, dd, ds, ni = ctx.encode_spans(b"".join(docs), doc_starts=starts)
    ids, off, spans = ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), ctx.d2h(ds, 16 * ni, np.uint64).reshape(-1, 2)
    assert [ids[off[d]:off[d + 1]].tolist() for d in range(len(docs))] == tok.encode_batch([d.decode() for d in docs])
    for kw in ({"row_len": 9, "bos_id": 7, "stride": 3}, {"row_len": 200, "eos_id": 8, "pad_left": True}, {"row_len": 1}):
        dev = ctx.layout_windows_to_host(di, ni, dd, len(docs), ds, pad_id=999, **kw)
        same(dev, ctx.layout_windows_to_host(ids, doc_starts=off[:-1], spans=spans, pad_id=999, **kw), kw)
        same(dev, wh.np_windows(ids, np.diff(off.astype(np.int64)), kw["row_len"], kw.get("stride", 0), 999, kw.get("bos_id"), kw.get("eos_id"),
                                kw.get("pad_left", False), spans), kw)
        same(ctx.layout_windows_to_host(di, ni, dd, len(docs), pad_id=999, **kw), dev[:4], (kw, "without spans"))
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), ids)  # the layout calls left the encoder's results alone
    assert np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), off)
    assert np.array_equal(ctx.d2h(ds, 16 * ni, np.uint64).reshape(-1, 2), spans)


def tok_check(tok, texts, what):
    as_texts = [texts.decode("utf-8")] if isinstance(texts, bytes) else texts
    cases = ({"max_length": 5, "stride": 2, "bos_id": 1}, {"max_length": 12, "stride": 10, "eos_id": 2, "padding_side": "left"},
             {"max_length": 3, "bos_id": 4_000_000_000, "eos_id": 0, "pad_id": 3}, {"max_length": 64, "stride": 16}, {"max_length": 1})
    for k, kw in enumerate(cases):
        for extra in ({}, {"offsets": "char"}, {"offsets": "byte"}) + (({"dropout": 0.1, "seed": 7},) if k < 2 else ()):
            got = tok.encode_array_windows(texts, **kw, **extra)
            exp = tok.encode_batch_windows(as_texts, **kw, **extra)
            assert len(got) == len(exp) == (5 if "offsets" in extra else 4), (what, kw, extra)
            assert got[0].dtype == np.uint32 and got[0].shape == (len(exp[0]), kw["max_length"]) and got[0].tolist() == exp[0], (what, kw, extra)
            for g, e in zip(got[1:4], exp[1:4]):
                assert g.dtype == np.uint32 and g.tolist() == e, (what, kw, extra)
            if "offsets" in extra:
                assert got[4].dtype == np.uint64 and got[4].shape == (len(exp[0]), kw["max_length"], 2), (what, kw, extra)
                assert got[4].tolist() == [[list(p) for p in row] for row in exp[4]], (what, kw, extra)


def test_through_the_tokenizer(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    for _idx, name, tok in setups:
        tok_check(tok, g9["texts"], name)
        tok_check(tok, g9["texts"][3].encode("utf-8"), (name, "a bytes buffer"))
        tok_check(tok, [], (name, "an empty sequence"))
        tok_check(tok, ["", ""], (name, "only empty documents"))
    base = next(tok for _i, name, tok in setups if name == "in_memory")
    rng = random.Random(3)
    for sp in SPECIALS:
        vocab = dict(base._vocab)
        for k, s in enumerate(sp):
            if k % 2 == 0:
                vocab.setdefault(s.encode(), 5000 + k)
        tok = BBPETokenizer(vocab=vocab, merges=list(base._merges), special_tokens=sp)
        texts = ["".join(rng.choice(sp + ["the ", "a", " it's", "é", ""]) for _ in range(rng.randint(0, 12))) for _ in range(40)]
        tok_check(tok, texts, sp)


def test_errors_leave_the_context_usable(ctx):
    from yet_another_bpe import _native

    ids, starts = wh.synth([3, 4])
    bad = [
        {"row_len": 0},                                                      # row_len <= n_added
        {"row_len": 1, "bos_id": 1},
        {"row_len": 2, "bos_id": 1, "eos_id": 2},
        {"row_len": 4, "stride": 4},                                         # stride >= row_len - n_added
        {"row_len": 4, "stride": 3, "eos_id": 2},
        {"row_len": 4, "stride": 0xFFFFFFFF},
        {"row_len": 4, "flags": _native.LAYOUT_TRUNC_LEFT},                  # flags of the other modes
        {"row_len": 4, "flags": _native.LAYOUT_DROP_LAST},
        {"row_len": 4, "flags": 0x20},                                       # an unknown flag
    ]
    for kw in bad:
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_windows(ids, doc_starts=starts, **kw)
        assert e.value.code == E_INVALID and len(str(e.value)) > len("yabpe error -1: "), kw
    for bad_starts in ([1, 3], [0, 5, 4], [0, 8]):  # not from 0, not ascending, past the ids
        with pytest.raises(_native.YabpeError) as e:
            ctx.layout_windows(ids, doc_starts=np.asarray(bad_starts, dtype=np.uint64), row_len=4)
        assert e.value.code == E_INVALID and "doc" in str(e.value)
    with pytest.raises(ValueError):  # not one span per id: refused by the binding
        ctx.layout_windows(ids, doc_starts=starts, spans=wh.synth_spans(6), row_len=4)
    same(*both(ctx, [3, 4], 4, 1, 1, None, False, True), "a good call after the bad ones")
    # 2^20 + 1 rows of 2^16 slots: more than 2^36 slots, found from the scan's total before any result is allocated
    with pytest.raises(_native.YabpeError) as e:
        ctx.layout_windows(np.zeros((1 << 20) + (1 << 16), np.uint32), row_len=1 << 16, stride=(1 << 16) - 1)
    assert e.value.code == E_CAPACITY and "2^36" in str(e.value)
    same(*both(ctx, [3, 4], 4, 1, 1, None, False), "a good call after the refused one")


def test_windows_stats(ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, 500).tolist()
    for (bos, eos), L, stride in ((wh.ADDED[0], 16, 4), (wh.ADDED[1], 25, 0), (wh.ADDED[3], 7, 4), (wh.ADDED[2], 64, 3)):
        n_added = (bos is not None) + (eos is not None)
        for spans in (False, True):
            got, exp = both(ctx, lens, L, stride, bos, eos, False, spans)
            same(got, exp, ("stats", L, stride))
            st = ctx.layout_stats()
            n_rows, n_multi, n_pad = wh.win_stats(lens, L, n_added, stride)
            assert n_rows == len(got[0]) and n_pad == n_rows * L - int(got[3].sum())
            assert (st["n_ids"], st["n_docs"], st["n_rows"], st["row_len"]) == (sum(lens), len(lens), n_rows, L), st
            assert (st["n_truncated_docs"], st["n_ids_dropped"], st["n_pad_slots"]) == (n_multi, 0, n_pad), st
            assert st["lengths_ms"] > 0 and st["write_ms"] > 0 and st["total_ms"] >= st["write_ms"], st


def test_results_outlive_the_next_encode(ctx):
    lens = [5, 0, 9]
    ids, starts = wh.synth(lens)
    sp = wh.synth_spans(len(ids))
    dr, dd, ds, dl, dsp, nr = ctx.layout_windows(ids, doc_starts=starts, spans=sp, row_len=4, stride=1, pad_id=wh.PAD, eos_id=2)
    exp = wh.np_windows(ids, lens, 4, 1, wh.PAD, None, 2, False, sp)
    ctx.encode_set_model(dict(IDENT), [], [], 0)
    ctx.encode_spans_to_host(b"other text " * 300)
    ctx.encode_free()
    assert nr == len(exp[0]) == 2 + 1 + 4
    got = (ctx.d2h(dr, 16 * nr, np.uint32).reshape(nr, 4),) + tuple(ctx.d2h(p, 4 * nr, np.uint32) for p in (dd, ds, dl))
    same(got + (ctx.d2h(dsp, 64 * nr, np.uint64).reshape(nr, 4, 2),), exp, "after the next encode")
    assert ctx.layout_windows(ids, doc_starts=starts, row_len=4)[4] == 0  # no spans in: none out
    ctx.layout_free()
    ctx.layout_free()  # (twice is fine)


def child():
    """Runs in the child process; the results the parent checks leave as one JSON line on stdout."""
    from yet_another_bpe import _native

    res = {}
    lens = child_lens()
    ids, starts = wh.synth(lens)
    ctx = _native.Context()
    mark("windows")
    got = ctx.layout_windows_to_host(ids, doc_starts=starts, row_len=100, stride=30, pad_id=5, bos_id=6)
    res["plain_ok"] = all(bool(np.array_equal(g, e)) for g, e in zip(got, wh.np_windows(ids, lens, 100, 30, 5, 6, None, False)))
    mark("windows_spans")
    sp = wh.synth_spans(len(ids))
    got = ctx.layout_windows_to_host(ids, doc_starts=starts, spans=sp, row_len=100, stride=30, pad_id=5, bos_id=6)
    res["spans_ok"] = all(bool(np.array_equal(g, e)) for g, e in zip(got, wh.np_windows(ids, lens, 100, 30, 5, 6, None, False, sp)))
    mark("windows_bad")
    try:
        ctx.layout_windows(ids, doc_starts=starts, row_len=100, stride=99, bos_id=6)
    except Exception as e:  # noqa: BLE001 (the parent checks the type)
        res["bad_err"] = [type(e).__name__, getattr(e, "code", None)]
    mark("close")
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def child_lens():
    return [3, 1] + np.random.default_rng(5).integers(0, 400, 2100).tolist() + [4000]


def test_every_traced_buffer_is_released():
    repo = helpers.GOLDEN.parent.parent
    code = (
        "import sys\n"
        f"sys.path[:0] = [{str(repo)!r}, {str(repo / 'yet-another-bpe_amd')!r}]\n"
        "from tests.test_gpu_encode_windows import child\n"
        "child()\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, YABPE_TRACE_ALLOC="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res == {"plain_ok": True, "spans_ok": True, "bad_err": ["YabpeError", E_INVALID]}
    live, section, sizes = {}, "start", {}
    for ln in out.stderr.splitlines():
        if ln.startswith("[mark] "):
            section = ln[len("[mark] "):]
        elif (m := ALLOC.match(ln)):
            assert m.group(2) not in live, f"{m.group(2)} handed out again in {section}; still held since {live[m.group(2)]}"
            live[m.group(2)] = section
            sizes.setdefault(section, []).append(int(m.group(3)))
        elif (m := FREE.match(ln)):
            live.pop(m.group(1), None)
    assert not live, f"never freed: {live}"
    # the driver's own buffers are in the trace: staged ids and starts, counters, row counts and their scan, the row records, the results
    lens = child_lens()
    n, nd = sum(lens), len(lens)
    n_rows = wh.win_stats(lens, 100, 1, 30)[0]
    for section in ("windows", "windows_spans"):
        for want in (4 * n, 8 * nd, 32, 8 * (nd + 1), 16 * n_rows, 4 * n_rows * 100):
            assert want in sizes[section], (section, want, sizes[section])
        assert sizes[section].count(4 * n_rows) == 3, (section, sizes[section])
    assert 16 * n in sizes["windows_spans"] and 16 * n_rows * 100 in sizes["windows_spans"]
    assert 16 * n_rows * 100 not in sizes["windows"] and len(sizes["windows_spans"]) == len(sizes["windows"]) + 2
    assert "windows_bad" not in sizes  # the bad call was refused before it allocated
