"""GPU: BBPETokenizer.encode_array_dropout (yabpe_encode_dropout) id for id and offset for offset against the plain-Python
encode_batch_dropout: pre-tokens of every length at which the kernels change their path (one byte, the 16-lane groups' edge
16 / 17, 32 / 33, the wave's edge 64 / 65 and the sequential walk beyond), multi-byte text, empty and identical documents,
specials with and without an id; p = 0 and p = 1, reproducibility over calls, contexts and seeds, the decode round trip, the
fixed-shape forms, malformed UTF-8, the C ABI's argument checks and statistics, and the allocation trace of a fresh process."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dropout_helpers as dh
from tests import encode_helpers, helpers
from tests.test_gpu_scratch_balance import ALLOC, FREE, mark
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
PS = [0.1, 0.5, 0.9]
SEEDS = [0, 0xDEADBEEFCAFEF00D]
E_INVALID = -1


@pytest.fixture(scope="module")
def toks(golden_dir, tmp_path_factory):
    """{name: tokenizer}: a few-hundred-merge model in memory, its lossy reload, a vocab lacking bytes, and with specials"""
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path_factory.mktemp("g9"))
    by = {(idx, name): tok for idx, name, tok in setups}
    plain = BBPETokenizer(vocab=dict(by[0, "in_memory"]._vocab), merges=list(by[0, "in_memory"]._merges), special_tokens=[])
    return {"plain": plain, "specials": dh.with_specials(plain), "from_file": by[0, "from_file"],
            "lacking": next(t for (_i, name), t in by.items() if name == "lacking_bytes_with_unk")}


def split(ids, off):
    ids, off = ids.tolist(), off.tolist()
    return [ids[off[d]:off[d + 1]] for d in range(len(off) - 1)]


@pytest.mark.parametrize("name", ["plain", "specials", "from_file", "lacking"])
def test_matches_plain_python(toks, name):
    tok = toks[name]
    docs = dh.documents(tok.special_tokens)
    assert len(docs) >= 3 and "" in docs and docs[0] == docs[2]
    for p in PS:
        for seed in SEEDS:
            exp = tok.encode_batch_dropout(docs, p, seed)
            ids, off = tok.encode_array_dropout(docs, p, seed)
            assert ids.dtype == np.uint32 and off.dtype == np.uint64 and len(off) == len(docs) + 1
            assert off.tolist() == np.concatenate(([0], np.cumsum([len(e) for e in exp]))).tolist(), (name, p, seed)
            got = split(ids, off)
            assert got == exp, (name, p, seed, next(d for d in range(len(docs)) if got[d] != exp[d]))
            assert got[0] != got[2]  # equal documents draw differently
    assert tok.encode_batch_device_dropout(docs, 0.5, 7) == tok.encode_batch_dropout(docs, 0.5, 7)
    one = docs[3].encode("utf-8")  # one bytes buffer is document 0
    assert tok.encode_array_dropout(one, 0.5, 7)[0].tolist() == tok.encode_dropout(docs[3], 0.5, 7)


def test_one_wave_per_word_form_gives_the_same_ids(toks):
    from yet_another_bpe import _native

    tok, docs = toks["specials"], dh.documents([dh.SP, dh.SP_NOID])
    ordered = sorted(tok.special_tokens, key=len, reverse=True)
    data, starts = tok._device_input(docs)
    with _native.Context() as ctx:
        ctx.encode_set_model(tok._vocab, tok._merges, ordered, tok._vocab.get(b"[UNK]", 0))
        ctx.set_option("dropout_pack", 0)
        ids, off = ctx.encode_dropout_to_host(data, tok._dropout_threshold(0.5), 3, doc_starts=starts)
    assert split(ids, off) == tok.encode_batch_dropout(docs, 0.5, 3)


def test_p0_is_encode_and_p1_is_per_byte(toks):
    for name in ("plain", "specials", "lacking"):
        tok = toks[name]
        docs = dh.documents(tok.special_tokens)
        ids0, off0 = tok.encode_array_dropout(docs, 0.0, 5)
        ids, off = tok.encode_array(docs)
        assert np.array_equal(ids0, ids) and np.array_equal(off0, off), name
        assert split(*tok.encode_array_dropout(docs, 2.0 ** -33, 5)) == split(ids, off), name  # T = 0
        assert split(*tok.encode_array_dropout(docs, 1.0, 5)) == [dh.per_byte(tok, d) for d in docs], name


def test_reproducible_over_calls_contexts_and_batches(toks):
    tok, docs = toks["specials"], dh.documents([dh.SP, dh.SP_NOID])
    a = tok.encode_array_dropout(docs, 0.5, 11)
    b = tok.encode_array_dropout(docs, 0.5, 11)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    other = BBPETokenizer(vocab=dict(tok._vocab), merges=list(tok._merges), special_tokens=list(tok.special_tokens))  # a context of its own
    c = other.encode_array_dropout(docs, 0.5, 11)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    d = tok.encode_array_dropout(docs, 0.5, 12)
    assert not np.array_equal(a[0], d[0])  # a changed seed
    first = split(*tok.encode_array_dropout(docs[:1] + ["unrelated text"], 0.5, 11))[0]  # document 0 in other company
    assert first == split(*a)[0]
    assert tok.encode_array_dropout([], 0.5, 1)[0].size == 0 and tok.encode_array_dropout([], 0.5, 1)[1].tolist() == [0]
    assert split(*tok.encode_array_dropout(["", ""], 0.5, 1)) == [[], []]


def test_decode_round_trip(toks):
    tok = toks["plain"]  # byte-complete
    docs = dh.documents()
    for p in PS:
        ids, off = tok.encode_array_dropout(docs, p, 4)
        text, toff = tok.decode_array(ids, off)
        data, toff = text.tobytes(), toff.tolist()
        assert [data[toff[d]:toff[d + 1]].decode("utf-8") for d in range(len(docs))] == docs, p


def test_fixed_shape_forms(toks):
    tok, docs = toks["specials"], dh.documents([dh.SP, dh.SP_NOID])
    for kw in (dict(max_length=None), dict(max_length=40, bos_id=1, eos_id=2, truncation="left", padding_side="left")):
        rows, lengths = tok.encode_array_padded(docs, dropout=0.5, seed=9, **kw)
        erows, elengths = tok.encode_batch_padded(docs, dropout=0.5, seed=9, **kw)
        assert rows.tolist() == erows and lengths.tolist() == elengths, kw
    for kw in (dict(seq_len=64), dict(seq_len=33, bos_id=1, eos_id=2, drop_last=True)):
        got = tok.encode_array_packed(docs, dropout=0.5, seed=9, **kw)
        exp = tok.encode_batch_packed(docs, dropout=0.5, seed=9, **kw)
        assert [g.tolist() for g in got] == list(exp), kw
    plain = tok.encode_array_packed(docs, 64)
    assert not np.array_equal(plain[0], tok.encode_array_packed(docs, 64, dropout=0.5, seed=9)[0])


def test_utf8_errors_and_arguments(toks):
    from yet_another_bpe import _native

    tok = toks["specials"]
    for b in [b"\x80", b"ab\xc3", b"\xe2\x82" + dh.SP.encode(), dh.SP.encode() + b"\x80", b"ok the" + b"\xc3\xa9\xa9"]:
        with pytest.raises(_native.Utf8Error) as e:
            tok.encode_array(b)
        with pytest.raises(_native.Utf8Error) as g:
            tok.encode_array_dropout(b, 0.5, 1)
        assert g.value.position == e.value.position, b
    for bad in (-0.1, 1.5, float("nan"), "0.5", None):
        with pytest.raises(ValueError):
            tok.encode_array_dropout(["a"], bad, 1)
    for bad in (-1, 1 << 64, 1.0):
        with pytest.raises(ValueError):
            tok.encode_array_dropout(["a"], 0.5, bad)
    ctx = tok._device()
    with pytest.raises(_native.YabpeError) as e:
        ctx.encode_dropout(b"the", (1 << 32) + 1, 0)
    assert e.value.code == E_INVALID
    ctx.encode_dropout(dh.documents([dh.SP])[-1].encode(), 1 << 31, 0)
    st = ctx.encode_stats()
    assert st["n_unique"] == 0 and st["pool_ms"] == 0 and st["n_specials"] == 4 and st["n_ids"] > 0 and st["total_ms"] > 0


TRACE_TEXT = ("ab " * 2731 + dh.SP + " ab" * 2731 + " " + "ab" * 40).encode()  # 16 KiB, over 2,048 pre-tokens, one long word


def child():
    """Runs in the child process (YABPE_TRACE_ALLOC=1): a good call, a malformed one and the release of the results."""
    from yet_another_bpe import _native

    vocab = {bytes([i]): i for i in range(256)}
    vocab[b"ab"] = 256
    vocab[dh.SP.encode()] = 257
    res = {}
    with _native.Context() as ctx:
        ctx.encode_set_model(vocab, [(b"a", b"b")], [dh.SP], 0)
        mark("warm")  # (the context builds its class table on the first encode and keeps it)
        ctx.encode(b"ab")
        ctx.encode_free()
        mark("dropout")
        ids, _off = ctx.encode_dropout_to_host(TRACE_TEXT, 1 << 31, 5)
        res["n_ids"] = int(ids.size)
        mark("dropout_broken")
        try:
            ctx.encode_dropout(TRACE_TEXT[:9001] + b"\xff" + TRACE_TEXT[9002:], 1 << 31, 5)
        except Exception as e:  # noqa: BLE001 (the parent checks the type)
            res["err"] = [type(e).__name__, getattr(e, "position", None)]
        mark("free")
        ctx.encode_free()
        mark("close")
    print("RESULT " + json.dumps(res), flush=True)


def test_every_traced_buffer_is_released():
    repo = helpers.GOLDEN.parent.parent
    code = (
        "import sys\n"
        f"sys.path[:0] = [{str(repo)!r}, {str(repo / 'yet-another-bpe_amd')!r}]\n"
        "from tests.test_gpu_encode_dropout import child\n"
        "child()\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, YABPE_TRACE_ALLOC="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["err"] == ["Utf8Error", 9001] and len(TRACE_TEXT) // 3 < res["n_ids"] < len(TRACE_TEXT)
    live, section, at_free = {}, "start", None
    for ln in out.stderr.splitlines():
        if ln.startswith("[mark] "):
            section = ln[len("[mark] "):]
            if section == "dropout_broken":
                held = dict(live)  # what outlives a good call: its two results
            if section == "close":
                at_free = dict(live)
        elif (m := ALLOC.match(ln)):
            assert m.group(2) not in live, f"{m.group(2)} handed out again in {section}; still held since {live[m.group(2)]}"
            live[m.group(2)] = section
        elif (m := FREE.match(ln)):
            live.pop(m.group(1), None)
    assert not live, f"never freed: {live}"
    assert sorted(held.values()).count("dropout") == 2, held  # ids and document offsets; every temporary went back
    assert at_free is not None and "dropout" not in at_free.values() and "dropout_broken" not in at_free.values(), at_free
