"""GPU: the fixed-shape batches (yabpe_layout_pad / yabpe_layout_pack).  Synthetic ids through Context.layout_*_to_host against
numpy (tests/layout_helpers.py, held against the plain-Python contract by tests/test_layout_model.py) over the grid of row
lengths, framing ids, sides and drop_last and the document lengths that take the kernels' other paths; the tokenizer's
encode_array_padded / encode_array_packed against encode_batch_padded / encode_batch_packed; device inputs, errors, stats,
results that outlive the next encode, 4 MiB of text checked with numpy alone, and the allocation trace of a fresh process."""
from __future__ import annotations

import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests import encode_helpers, helpers
from tests import layout_helpers as lh
from tests.test_gpu_pretok import SPECIALS
from tests.test_gpu_scratch_balance import ALLOC, FREE, mark
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
IDENT = {bytes([i]): i for i in range(256)}
E_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from yet_another_bpe import _native

    with _native.Context() as c:
        yield c


def same(got, exp, what):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.dtype == np.uint32 and g.shape == e.shape, (what, g.shape, e.shape)
        assert np.array_equal(g, e), (what, np.argwhere(g != e)[:5].tolist())


def pad_both(ctx, lens, L, bos, eos, tl, pl, pad=lh.PAD):
    ids, starts = lh.synth(lens)
    got = ctx.layout_pad_to_host(ids, doc_starts=starts, row_len=L or 0, pad_id=pad, bos_id=bos, eos_id=eos, trunc_left=tl, pad_left=pl)
    return got, lh.np_pad(ids, lens, L, pad, bos, eos, tl, pl)


def pack_both(ctx, lens, L, bos, eos, dl, pad=lh.PAD):
    ids, starts = lh.synth(lens)
    got = ctx.layout_pack_to_host(ids, doc_starts=starts, row_len=L, pad_id=pad, bos_id=bos, eos_id=eos, drop_last=dl)
    return got, lh.np_pack(ids, lens, L, pad, bos, eos, dl)


def test_padded_grid(ctx):
    for L, bos, eos, tl, pl in lh.pad_cases():
        same(*pad_both(ctx, lh.grid_lengths(L, (bos is not None) + (eos is not None)), L, bos, eos, tl, pl), (L, bos, eos, tl, pl))


def test_packed_grid(ctx):
    for L, bos, eos, dl in lh.pack_cases():
        same(*pack_both(ctx, lh.grid_lengths(L, (bos is not None) + (eos is not None)), L, bos, eos, dl), (L, bos, eos, dl))


def test_other_paths(ctx):
    for name, lens in lh.special_length_sets().items():
        for (bos, eos), L in ((lh.ADDED[0], 64), (lh.ADDED[2], 33), (lh.ADDED[3], 2048)):
            for dl in (False, True):
                same(*pack_both(ctx, lens, L, bos, eos, dl), (name, L, dl))
            same(*pad_both(ctx, lens, L, bos, eos, True, False), (name, L))
    lens = [64] * 8  # a stream that is an exact multiple of the row: no pad slot
    got, exp = pack_both(ctx, lens, 128, None, None, False)
    same(got, exp, "exact multiple")
    assert got[0].shape == (4, 128) and not (got[1] == lh.NO_DOC).any() and ctx.layout_stats()["n_pad_slots"] == 0
    for dl in (False, True):  # a stream of length 0 from only empty documents: zero rows
        got, exp = pack_both(ctx, [0, 0, 0], 8, None, None, dl)
        same(got, exp, "empty stream")
        assert got[0].shape == (0, 8)
    ids = np.arange(10, dtype=np.uint32)  # one document, without document starts at all
    same(ctx.layout_pack_to_host(ids, row_len=4, pad_id=1), lh.np_pack(ids, [10], 4, 1, None, None, False), "n_docs = 1")
    same(ctx.layout_pad_to_host(ids, row_len=12, pad_id=1, eos_id=2), lh.np_pad(ids, [10], 12, 1, None, 2, False, False), "n_docs = 1")
    big = 0xFFFFFFFE  # ids next to the top of u32 come back unchanged
    same(*pack_both(ctx, [3, 0, 6], 4, big, big, False, pad=big), "0xFFFFFFFE")
    got, exp = pad_both(ctx, [3, 0, 6], 6, big, big, False, True, pad=big)
    same(got, exp, "0xFFFFFFFE")
    assert got[0][1].tolist() == [big] * 6 and got[1].tolist() == [5, 2, 6]


def test_longest_sequence_as_row_length(ctx):
    for bos, eos in lh.ADDED:
        n_added = (bos is not None) + (eos is not None)
        for lens in ([3, 0, 11, 5], [0, 0], [0], [1], [2] * 300 + [700] + [1] * 300):
            for pl in (False, True):
                got, exp = pad_both(ctx, lens, None, bos, eos, False, pl)
                same(got, exp, (lens[:4], bos, eos, pl))
                assert got[0].shape == (len(lens), max(lens) + n_added)  # all empty: L = n_added
                assert ctx.layout_stats()["row_len"] == max(lens) + n_added and ctx.layout_stats()["n_truncated_docs"] == 0


def test_device_inputs(ctx):
    """Context.encode's device pointers passed straight in give what the host copies of the same ids give."""
    tok = BBPETokenizer(vocab={**IDENT, b"th": 256, b"he": 257}, merges=[(b"t", b"h"), (b"h", b"e")])
    docs = [b"the other thing", b"", b"he then", b"x" * 100, b""]
    starts = np.cumsum([0] + [len(d) for d in docs[:-1]]).astype(np.uint64)
    ctx.encode_set_model(tok._vocab, tok._merges, [], 0)
    di, dd, ni = ctx.encode(b"".join(docs), doc_starts=starts)
    ids, off = ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)
    assert [ids[off[d]:off[d + 1]].tolist() for d in range(len(docs))] == tok.encode_batch([d.decode() for d in docs])
    for kw in ({"row_len": 0}, {"row_len": 9, "bos_id": 7, "trunc_left": True}, {"row_len": 200, "eos_id": 8, "pad_left": True}):
        dev = ctx.layout_pad_to_host(di, ni, dd, len(docs), pad_id=999, **kw)
        same(dev, ctx.layout_pad_to_host(ids, doc_starts=off[:-1], pad_id=999, **kw), kw)
    for kw in ({"row_len": 16}, {"row_len": 7, "eos_id": 8, "drop_last": True}, {"row_len": 1, "bos_id": 1, "eos_id": 2}):
        dev = ctx.layout_pack_to_host(di, ni, dd, len(docs), pad_id=999, **kw)
        same(dev, ctx.layout_pack_to_host(ids, doc_starts=off[:-1], pad_id=999, **kw), kw)
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), ids)  # the layout calls left the encoder's results alone
    assert np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), off)


def tok_check(tok, texts, what):
    for kw in ({}, {"max_length": 5, "bos_id": 1}, {"max_length": 12, "eos_id": 2, "truncation": "left", "padding_side": "left"},
               {"max_length": 2, "bos_id": 4_000_000_000, "eos_id": 0, "pad_id": 3}, {"max_length": 0}):
        rows, lengths = tok.encode_array_padded(texts, **kw)
        erows, elen = tok.encode_batch_padded([texts.decode("utf-8")] if isinstance(texts, bytes) else texts, **kw)
        assert rows.dtype == np.uint32 and lengths.dtype == np.uint32 and lengths.tolist() == elen, (what, kw)
        assert rows.shape == (len(erows), len(erows[0]) if erows else kw.get("max_length") or 0) and rows.tolist() == erows, (what, kw)
    for kw in ({"seq_len": 8}, {"seq_len": 3, "eos_id": 2, "drop_last": True}, {"seq_len": 64, "bos_id": 1, "eos_id": 2, "pad_id": 9}):
        got = tok.encode_array_packed(texts, **kw)
        exp = tok.encode_batch_packed([texts.decode("utf-8")] if isinstance(texts, bytes) else texts, **kw)
        for g, e in zip(got, exp):
            assert g.dtype == np.uint32 and g.shape == (len(e), kw["seq_len"]) and g.tolist() == e, (what, kw)


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

    ids, starts = lh.synth([3, 4])
    bad = [
        (ctx.layout_pad, {"row_len": 4, "flags": 0x20}),                        # an unknown flag
        (ctx.layout_pack, {"row_len": 4, "flags": 0x100}),
        (ctx.layout_pad, {"row_len": 1, "bos_id": 1, "eos_id": 2}),             # row_len < n_added
        (ctx.layout_pack, {"row_len": 0}),                                      # a packed row of no slots
        (ctx.layout_pad, {"row_len": 4, "flags": _native.LAYOUT_DROP_LAST}),    # flags of the other mode
        (ctx.layout_pack, {"row_len": 4, "flags": _native.LAYOUT_TRUNC_LEFT}),
        (ctx.layout_pack, {"row_len": 4, "flags": _native.LAYOUT_PAD_LEFT}),
    ]
    for call, kw in bad:
        with pytest.raises(_native.YabpeError) as e:
            call(ids, doc_starts=starts, **kw)
        assert e.value.code == E_INVALID and len(str(e.value)) > len("yabpe error -1: "), kw
    for bad_starts in ([1, 3], [0, 5, 4], [0, 8]):  # not from 0, not ascending, past the ids
        for call in (ctx.layout_pad, ctx.layout_pack):
            with pytest.raises(_native.YabpeError) as e:
                call(ids, doc_starts=np.asarray(bad_starts, dtype=np.uint64), row_len=4)
            assert e.value.code == E_INVALID and "doc" in str(e.value)
    same(*pad_both(ctx, [3, 4], 4, 1, None, False, False), "a good call after the bad ones")
    same(*pack_both(ctx, [3, 4], 4, 1, None, False), "a good call after the bad ones")


def test_results_outlive_the_next_encode(ctx):
    ids, starts = lh.synth([5, 0, 9])
    dr, dl, L = ctx.layout_pad(ids, doc_starts=starts, row_len=6, pad_id=lh.PAD, eos_id=2)
    exp = lh.np_pad(ids, [5, 0, 9], 6, lh.PAD, None, 2, False, False)
    ctx.encode_set_model(dict(IDENT), [], [], 0)
    ctx.encode_to_host(b"other text " * 300)
    ctx.encode_free()
    assert L == 6 and np.array_equal(ctx.d2h(dr, 4 * 3 * 6, np.uint32).reshape(3, 6), exp[0]) and np.array_equal(ctx.d2h(dl, 12, np.uint32), exp[1])
    di, dd, dp, nr = ctx.layout_pack(ids, doc_starts=starts, row_len=4, pad_id=lh.PAD, eos_id=2)
    exp = lh.np_pack(ids, [5, 0, 9], 4, lh.PAD, None, 2, False)
    ctx.encode_to_host(b"and more " * 300)
    for p, e in zip((di, dd, dp), exp):
        assert nr == 5 and np.array_equal(ctx.d2h(p, 4 * nr * 4, np.uint32).reshape(nr, 4), e)
    ctx.layout_free()
    ctx.layout_free()  # (twice is fine)


def test_layout_stats(ctx):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, 500).tolist()
    for (bos, eos), L in ((lh.ADDED[0], 16), (lh.ADDED[1], 25), (lh.ADDED[3], 7)):
        n_added = (bos is not None) + (eos is not None)
        same(*pad_both(ctx, lens, L, bos, eos, False, False), ("stats", L))
        st = ctx.layout_stats()
        assert (st["n_truncated_docs"], st["n_ids_dropped"], st["n_pad_slots"]) == lh.pad_stats(lens, L, n_added), st
        assert (st["n_ids"], st["n_docs"], st["n_rows"], st["row_len"]) == (sum(lens), len(lens), len(lens), L), st
        assert st["lengths_ms"] > 0 and st["write_ms"] > 0 and st["total_ms"] >= st["write_ms"], st
        total = sum(lens) + n_added * len(lens)
        for dl in (False, True):
            same(*pack_both(ctx, lens, L, bos, eos, dl), ("stats", L, dl))
            st = ctx.layout_stats()
            n_rows = total // L if dl else -(-total // L)
            assert (st["n_rows"], st["row_len"], st["n_truncated_docs"]) == (n_rows, L, 0), st
            assert st["n_ids_dropped"] == (total - n_rows * L if dl else 0) and st["n_pad_slots"] == (0 if dl else n_rows * L - total), st
            assert st["write_ms"] > 0, st


def test_scale_without_python_per_token():
    from yet_another_bpe import _native

    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, 4 << 20)
        vocab, merges, trained = encode_helpers.train_on_device(gen, tb, tn, 2000)
        trained.close()
        data = gen.d2h(tb, tn).tobytes()
    cut = [0]  # 64 documents, cut at character starts
    for k in range(1, 64):
        p = k * tn // 64
        while data[p] & 0xC0 == 0x80:
            p += 1
        cut.append(p)
    docs = [data[a:b].decode("utf-8") for a, b in zip(cut, cut[1:] + [tn])]
    tok = BBPETokenizer(vocab=vocab, merges=merges)
    ids, off = tok.encode_array(docs)
    o = off.astype(np.int64)
    lens = np.diff(o)
    assert len(ids) > 500_000 and lens.min() > 4096
    # padded: every row is the head (or the tail) of its document, through fancy indexing
    L = 4096
    for tl in (False, True):
        rows, kept = tok.encode_array_padded(docs, L, bos_id=1, pad_id=0, truncation="left" if tl else "right")
        assert rows.shape == (64, L) and np.all(kept == L) and np.all(rows[:, 0] == 1)
        first = (o[1:] - (L - 1)) if tl else o[:-1]
        assert np.array_equal(rows[:, 1:], ids[first[:, None] + np.arange(L - 1)[None, :]])
    rows, kept = tok.encode_array_padded(docs, eos_id=2, pad_id=7)  # no cut: the longest document sets the row
    assert rows.shape == (64, lens.max() + 1) and np.array_equal(kept, lens + 1)
    col = np.arange(rows.shape[1])[None, :]
    assert np.array_equal(rows[col < lens[:, None]], ids) and np.all(rows[col == lens[:, None]] == 2) and np.all(rows[col > lens[:, None]] == 7)
    # packed: the stream, the documents and the positions
    S = 2048
    pids, pdoc, ppos = tok.encode_array_packed(docs, S, eos_id=2, pad_id=7)
    total = len(ids) + 64
    assert pids.shape == (-(-total // S), S)
    pids, pdoc, ppos = pids.ravel(), pdoc.ravel(), ppos.ravel()
    real = pdoc != lh.NO_DOC
    assert real.sum() == total and real[:total].all() and np.all(pids[~real] == 7) and np.all(ppos[~real] == 0)
    seq = lens + 1
    assert np.array_equal(pdoc[real], np.repeat(np.arange(64), seq))
    assert np.array_equal(ppos[real], np.arange(total) - np.repeat(np.cumsum(seq) - seq, seq))
    last = ppos[real] == np.repeat(seq, seq) - 1
    assert np.array_equal(pids[real][~last], ids) and np.all(pids[real][last] == 2)


def child():
    """Runs in the child process; the results the parent checks leave as one JSON line on stdout."""
    from yet_another_bpe import _native

    res = {}
    lens = lh.special_length_sets()["a window larger than the stage"]
    ids, starts = lh.synth(lens)
    ctx = _native.Context()
    mark("layout_pad")
    rows, kept = ctx.layout_pad_to_host(ids, doc_starts=starts, row_len=0, pad_id=5, bos_id=6)
    res["pad_ok"] = bool(np.array_equal(rows, lh.np_pad(ids, lens, None, 5, 6, None, False, False)[0]) and kept.sum() == len(ids) + len(lens))
    mark("layout_pack")
    got = ctx.layout_pack_to_host(ids, doc_starts=starts, row_len=100, pad_id=5, eos_id=6)
    res["pack_ok"] = all(bool(np.array_equal(g, e)) for g, e in zip(got, lh.np_pack(ids, lens, 100, 5, None, 6, False)))
    mark("layout_bad")
    try:
        ctx.layout_pack(ids, doc_starts=starts, row_len=0)
    except Exception as e:  # noqa: BLE001 (the parent checks the type)
        res["bad_err"] = [type(e).__name__, getattr(e, "code", None)]
    mark("close")
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def test_every_traced_buffer_is_released():
    repo = helpers.GOLDEN.parent.parent
    code = (
        "import sys\n"
        f"sys.path[:0] = [{str(repo)!r}, {str(repo / 'yet-another-bpe_amd')!r}]\n"
        "from tests.test_gpu_encode_layout import child\n"
        "child()\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, YABPE_TRACE_ALLOC="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res == {"pad_ok": True, "pack_ok": True, "bad_err": ["YabpeError", E_INVALID]}
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
    # the drivers' own buffers are in the trace: staged ids and starts, the counters, the results
    lens = lh.special_length_sets()["a window larger than the stage"]
    n, nd = sum(lens), len(lens)
    assert nd > 2049
    for want in (4 * n, 8 * nd, 32, 4 * nd, 4 * nd * (max(lens) + 1)):
        assert want in sizes["layout_pad"], (want, sizes["layout_pad"])
    n_slots = -(-(n + nd) // 100) * 100
    assert sizes["layout_pack"].count(4 * n_slots) == 3 and 8 * (nd + 1) in sizes["layout_pack"], sizes["layout_pack"]
    assert "layout_bad" not in sizes  # the bad call was refused before it allocated
