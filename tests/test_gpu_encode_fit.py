"""GPU: whole documents packed into rows (yabpe_layout_fit).  Synthetic ids through Context.layout_fit_to_host against the
plain-Python contract BBPETokenizer.encode_batch_fit run on the same ids (tests/fit_helpers.py; the contract is held against a
literal best-fit decreasing by tests/test_fit_model.py): every array exactly, and the call's counters; the document lengths
that take the kernels' other paths; device inputs; every refusal, with nothing allocated; then the tokenizer's encode_array_fit
against encode_batch_fit on the golden corpus, with and without dropout."""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import encode_helpers, helpers
from tests import fit_helpers as fh
from tests import layout_helpers as lh
from tests.test_gpu_scratch_balance import ALLOC, FREE, mark
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
IDENT = {bytes([i]): i for i in range(256)}
E_INVALID = -1
BOS, EOS = 70001, 70002


def lengths(name):
    rng = np.random.default_rng(7)
    return {
        "hand": [6, 6, 6, 2, 2, 2],
        "three-way": [5] * 5 + [2] * 5,                                    # rows of one shape: two filled, one partly, two untouched
        "pieces": rng.integers(1, 41, 700).tolist(),                       # more than 4,096 slots, rows not aligned to 4
        "stage": [1] * 6000 + [2] * 40,                                    # more places in a piece than the LDS stage holds
        "digit2": rng.integers(1, 301, 1500).tolist(),                     # a second radix digit, a last sort tile that is not full
        "digit3": [70000, 65536, 4464, 1, 300, 69999],                     # a third radix digit
        "equal": [3] * 1000,                                               # equal keys: ascending d
        "long": [50, 3, 0, 41, 40, 39, 38, 37, 120, 1],                    # longer than the row
        "tiny": [0, 4, 1, 0, 2],
        "empty": [0, 0, 0],
    }[name]


CASES = [  # (lengths, C, bos, eos)
    ("hand", 10, None, None), ("three-way", 9, None, None), ("pieces", 37, None, EOS), ("pieces", 37, None, None), ("stage", 5000, None, None),
    ("digit2", 300, None, None), ("digit3", 70000, None, None), ("equal", 10, None, None), ("long", 40, BOS, None), ("long", 40, None, EOS),
    ("long", 40, BOS, EOS), ("tiny", 2, BOS, EOS), ("tiny", 1, None, EOS), ("tiny", 1, None, None), ("empty", 8, None, None), ("empty", 8, BOS, None),
]


@functools.lru_cache(maxsize=None)
def expected(name, C, bos, eos):
    """the contract on the case's ids, computed once (the arrays are shared: nobody writes to them)"""
    return fh.contract(lengths(name), C, bos, eos)


@pytest.fixture(scope="module")
def ctx():
    from yet_another_bpe import _native

    with _native.Context() as c:
        yield c


def same(got, exp, what):
    assert len(got) == len(exp) == 4
    for g, e in zip(got, exp):
        assert g.dtype == np.uint32 and g.shape == e.shape, (what, g.shape, e.shape)
        assert np.array_equal(g, e), (what, np.argwhere(g != e)[:5].tolist())


@pytest.mark.parametrize("name,C,bos,eos", CASES)
def test_against_the_contract(ctx, name, C, bos, eos):
    lens = lengths(name)
    ids, starts = lh.synth(lens)
    exp = expected(name, C, bos, eos)
    same(ctx.layout_fit_to_host(ids, doc_starts=starts, row_len=C, pad_id=lh.PAD, bos_id=bos, eos_id=eos), exp, (name, C, bos, eos))
    st = ctx.layout_stats()
    n_added = (bos is not None) + (eos is not None)
    assert (st["n_ids"], st["n_docs"], st["n_rows"], st["row_len"]) == (sum(lens), len(lens), len(exp[3]), C), st
    assert (st["n_truncated_docs"], st["n_ids_dropped"], st["n_pad_slots"]) == fh.stats(lens, C, n_added, len(exp[3])), st
    assert st["total_ms"] >= st["write_ms"] >= 0 and st["lengths_ms"] > 0, st


def test_cases_take_the_paths_they_name():
    assert expected("pieces", 37, None, EOS)[0].size > 4096 and expected("pieces", 37, None, EOS)[0].shape[0] * 37 % 4
    assert max(len(s) for s in fh.row_shapes(*expected("stage", 5000, None, None)[1:3])) > 1024  # (the stage holds 1,024 places)
    assert len(lengths("digit2")) % 2048 and max(lengths("digit2")) >= 256 and max(lengths("digit3")) >= 65536
    used = expected("three-way", 9, None, None)[3].tolist()
    assert used == [9, 9, 7, 5, 5]
    assert expected("hand", 10, None, None)[1][:, 6:].tolist() == [[3, 3, 4, 4], [5, 5, lh.NO_DOC, lh.NO_DOC], [lh.NO_DOC] * 4]
    assert expected("equal", 10, None, None)[1][:, 0:9:3].ravel()[:1000].tolist() == list(range(1000))  # equal keys: ascending d


def test_no_documents_and_one_document(ctx):
    got = ctx.layout_fit_to_host(np.zeros(0, np.uint32), doc_starts=np.zeros(0, np.uint64), row_len=8)
    assert [g.shape for g in got] == [(0, 8)] * 3 + [(0,)] and ctx.layout_stats()["n_rows"] == 0 and ctx.layout_stats()["row_len"] == 8
    ids = np.arange(10, dtype=np.uint32)  # one document, without document starts at all
    same(ctx.layout_fit_to_host(ids, row_len=12, pad_id=1, eos_id=2), fh.contract([10], 12, None, 2, pad=1), "n_docs = 1")
    big = 0xFFFFFFFE  # ids next to the top of u32 come back unchanged
    lens = [3, 0, 6]
    got = ctx.layout_fit_to_host(*lh.synth(lens)[:1], doc_starts=lh.synth(lens)[1], row_len=8, pad_id=big, bos_id=big, eos_id=big)
    same(got, fh.contract(lens, 8, big, big, pad=big), "0xFFFFFFFE")


def test_device_inputs(ctx):
    """Context.encode's device pointers passed straight in give what the host copies of the same ids give, and stay as they are."""
    tok = BBPETokenizer(vocab={**IDENT, b"th": 256, b"he": 257}, merges=[(b"t", b"h"), (b"h", b"e")])
    docs = [b"the other thing", b"", b"he then", b"x" * 100, b"", b"the"]
    starts = np.cumsum([0] + [len(d) for d in docs[:-1]]).astype(np.uint64)
    ctx.encode_set_model(tok._vocab, tok._merges, [], 0)
    di, dd, ni = ctx.encode(b"".join(docs), doc_starts=starts)
    ids, off = ctx.d2h(di, 4 * ni, np.uint32), ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64)
    lens = np.diff(off.astype(np.int64)).tolist()
    for kw in ({"row_len": 16}, {"row_len": 7, "eos_id": 8}, {"row_len": 2, "bos_id": 1, "eos_id": 2}, {"row_len": 128, "bos_id": 5}):
        dev = ctx.layout_fit_to_host(di, ni, dd, len(docs), pad_id=999, **kw)
        same(dev, ctx.layout_fit_to_host(ids, doc_starts=off[:-1], pad_id=999, **kw), kw)
        same(dev, fh.contract(lens, kw["row_len"], kw.get("bos_id"), kw.get("eos_id"), pad=999, ids=ids), kw)
    assert np.array_equal(ctx.d2h(di, 4 * ni, np.uint32), ids)  # the layout calls left the encoder's results alone
    assert np.array_equal(ctx.d2h(dd, 8 * (len(docs) + 1), np.uint64), off)


def test_results_outlive_the_next_encode(ctx):
    lens = [5, 0, 9, 2]
    ids, starts = lh.synth(lens)
    di, dd, dp, du, nr = ctx.layout_fit(ids, doc_starts=starts, row_len=10, pad_id=lh.PAD, eos_id=2)
    exp = fh.contract(lens, 10, None, 2)
    ctx.encode_set_model(dict(IDENT), [], [], 0)
    ctx.encode_to_host(b"other text " * 300)
    assert nr == len(exp[3])
    for p, e in zip((di, dd, dp), exp):
        assert np.array_equal(ctx.d2h(p, 4 * nr * 10, np.uint32).reshape(nr, 10), e)
    assert np.array_equal(ctx.d2h(du, 4 * nr, np.uint32), exp[3])
    ctx.layout_free()
    ctx.layout_free()  # (twice is fine)


BAD = [  # (keywords, code)
    ({"row_len": 4, "flags": 0x20}, E_INVALID),              # an unknown flag
    ({"row_len": 4, "flags": 0x04}, E_INVALID),              # flags of the other layouts: TRUNC_LEFT, PAD_LEFT, DROP_LAST
    ({"row_len": 4, "flags": 0x08}, E_INVALID),
    ({"row_len": 4, "flags": 0x10}, E_INVALID),
    ({"row_len": 0}, E_INVALID),                             # a row of no slots
    ({"row_len": 1, "bos_id": 1, "eos_id": 2}, E_INVALID),   # row_len < n_added
    ({"row_len": 1 << 24}, E_INVALID),                       # past the sort keys
]


def refusals(ctx):
    """every refusal -> [[exception type, code], ...]"""
    from yet_another_bpe import _native

    ids, starts = lh.synth([3, 4])
    seen = []
    calls = [(starts, kw) for kw, _code in BAD] + [(np.asarray(s, dtype=np.uint64), {"row_len": 4}) for s in ([1, 3], [0, 5, 4], [0, 8])]
    for st, kw in calls:
        try:
            ctx.layout_fit(ids, doc_starts=st, **kw)
            seen.append(["no error", 0])
        except _native.YabpeError as e:
            seen.append([type(e).__name__, e.code, len(str(e)) > len("yabpe error -1: ")])
    return seen


def test_errors_leave_the_context_usable(ctx):
    assert refusals(ctx) == [["YabpeError", code, True] for _kw, code in BAD] + [["YabpeError", E_INVALID, True]] * 3
    lens = lengths("hand")
    ids, starts = lh.synth(lens)
    same(ctx.layout_fit_to_host(ids, doc_starts=starts, row_len=10, pad_id=lh.PAD), expected("hand", 10, None, None), "a good call after the bad ones")


def child():
    """Runs in the child process; the results the parent checks leave as one JSON line on stdout."""
    from yet_another_bpe import _native

    res = {}
    lens = lengths("pieces")
    ids, starts = lh.synth(lens)
    ctx = _native.Context()
    mark("layout_fit")
    got = ctx.layout_fit_to_host(ids, doc_starts=starts, row_len=37, pad_id=lh.PAD, eos_id=EOS)
    res["fit_ok"] = all(bool(np.array_equal(g, e)) for g, e in zip(got, expected("pieces", 37, None, EOS)))
    mark("layout_bad")
    res["bad"] = refusals(ctx)
    mark("close")
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def test_refusals_allocate_nothing_and_every_buffer_is_released():
    repo = helpers.GOLDEN.parent.parent
    code = (
        "import sys\n"
        f"sys.path[:0] = [{str(repo)!r}, {str(repo / 'yet-another-bpe_amd')!r}]\n"
        "from tests.test_gpu_encode_fit import child\n"
        "child()\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, YABPE_TRACE_ALLOC="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res == {"fit_ok": True, "bad": [["YabpeError", code, True] for _kw, code in BAD] + [["YabpeError", E_INVALID, True]] * 3}
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
    # the driver's own buffers are in the trace: staged ids and starts, keys, histogram, counters, the results
    lens = lengths("pieces")
    n, nd, n_rows = sum(lens), len(lens), len(expected("pieces", 37, None, EOS)[3])
    for want in (4 * n, 8 * nd, 4 * nd, 4 * 38, 32, 4 * n_rows):
        assert want in sizes["layout_fit"], (want, sizes["layout_fit"])
    assert sizes["layout_fit"].count(4 * n_rows * 37) == 3, sizes["layout_fit"]
    assert "layout_bad" not in sizes  # every bad call was refused before it allocated


def test_through_the_tokenizer(golden_dir, tmp_path):
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    tok = next(tok for _i, name, tok in setups if name == "in_memory")
    lines = (golden_dir / "corpus.en").read_text(encoding="utf-8").splitlines()[:400]
    assert len(lines) > 100
    for texts in (lines, lines[:1], ["", ""], []):
        for kw in ({"seq_len": 64}, {"seq_len": 33, "eos_id": 2, "pad_id": 9}, {"seq_len": 512, "bos_id": 1, "eos_id": 2},
                   {"seq_len": 16, "bos_id": 4_000_000_000}, {"seq_len": 48, "eos_id": 2, "dropout": 0.25, "seed": 5}):
            got = tok.encode_array_fit(texts, **kw)
            exp = tok.encode_batch_fit(texts, **kw)
            assert all(g.dtype == np.uint32 for g in got) and got[3].tolist() == exp[3], (len(texts), kw)
            for g, e in zip(got[:3], exp[:3]):
                assert g.shape == (len(e), kw["seq_len"]) and g.tolist() == e, (len(texts), kw)
    with_drop = tok.encode_array_fit(lines, 48, eos_id=2, dropout=0.25, seed=5)
    assert not np.array_equal(with_drop[0], tok.encode_array_fit(lines, 48, eos_id=2)[0])  # (the draw did change the ids)
