"""GPU: the device encoder with spans (yabpe_encode_spans through BBPETokenizer.encode_array_with_offsets) against the
plain-Python contract encode_batch_with_offsets, in bytes and in characters -- G9's set-ups, random strings with nested /
overlapping specials (half of them without an id), both paths of the words kernel and their boundary, document and granule
boundaries, and 4 MiB of synthetic text checked with numpy alone."""
from __future__ import annotations

import random

import numpy as np
import pytest

from tests import encode_helpers
from tests.test_gpu_pretok import SPECIALS
from yet_another_bpe.tokenizer import BBPETokenizer

pytestmark = pytest.mark.gpu
UNITS = ("byte", "char")
IDENT = {bytes([i]): i for i in range(256)}


def flat(batch):
    """[(ids, spans)] per document -> (ids, doc_off, spans) as encode_array_with_offsets lays them out"""
    ids = [i for d in batch for i in d[0]]
    spans = [p for d in batch for p in d[1]]
    off = np.cumsum([0] + [len(d[0]) for d in batch])
    return np.asarray(ids, dtype=np.uint32), off.astype(np.uint64), np.asarray(spans, dtype=np.uint64).reshape(-1, 2)


def check(tok, texts, what=None):
    plain_ids, plain_off = tok.encode_array(texts)
    for unit in UNITS:
        ids, off, spans = tok.encode_array_with_offsets(texts, unit)
        assert ids.dtype == np.uint32 and off.dtype == np.uint64 and spans.dtype == np.uint64 and spans.shape == (len(ids), 2)
        eids, eoff, espans = flat(tok.encode_batch_with_offsets(texts, unit))
        assert np.array_equal(ids, eids) and np.array_equal(off, eoff), (what, unit)
        assert np.array_equal(spans, espans), (what, unit, np.flatnonzero((spans != espans).any(axis=1))[:5])
        assert np.array_equal(ids, plain_ids) and np.array_equal(off, plain_off), (what, unit)


def test_g9_setups(golden_dir, tmp_path):
    g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    texts = g9["texts"]
    for _idx, name, tok in setups:
        check(tok, texts, name)
        for unit in UNITS:
            assert tok.encode_batch_device_with_offsets(texts, unit) == tok.encode_batch_with_offsets(texts, unit), (name, unit)
            for t in texts[:12]:  # a bytes buffer: one document
                ids, off, spans = tok.encode_array_with_offsets(t.encode("utf-8"), unit)
                eids, espans = tok.encode_with_offsets(t, unit)
                assert ids.tolist() == eids and off.tolist() == [0, len(eids)] and [tuple(p) for p in spans.tolist()] == espans, (name, t, unit)


def test_random_strings(golden_dir, tmp_path):
    _g9, setups = encode_helpers.g9_setups(golden_dir, tmp_path)
    base = next(tok for _i, name, tok in setups if name == "in_memory")
    rng = random.Random(21)
    alphabets = ["ab '", "a1 .'s\n", "'stdmlvre x", " \t\n\r\x0b\x0c\x85  a1.", "<|endoftext|> a's", "<s>x' ", "é中\U0001F600a 1'", "[PAD][UNK] ab",
                 "it's ", "<>", "the quick ", "er in on an "]
    for sp in SPECIALS + [["'s", "'"], ["<", "<<", "<<<"], ["aaa", "aa", "a"], [" ", "  "], ["a'll"], ["<|x|>", "<|x|><|y|>", "<|y|>"]]:
        vocab = dict(base._vocab)
        for k, s in enumerate(sp):
            if k % 2 == 0:
                vocab.setdefault(s.encode(), 5000 + k)
        tok = BBPETokenizer(vocab=vocab, merges=list(base._merges), special_tokens=sp)
        strings = ["".join(rng.choice(al) for _ in range(rng.randint(0, 40))) for al in (rng.choice(alphabets) for _ in range(1500))]
        strings += [" " * rng.randint(60, 200), "the" * rng.randint(20, 90)]
        for unit in UNITS:
            assert tok.encode_batch_device_with_offsets(strings, unit) == tok.encode_batch_with_offsets(strings, unit), (sp, unit)


def test_edges():
    merges = [(b"a", b"b"), (b"ab", b"a"), (b"b", b"b"), (b"\xc3", b"\xa9"), (b"\xc3\xa9", b"\xc3\xa9"), (b" ", b" ")]
    vocab = dict(IDENT)
    for l, r in merges[:-1]:  # "  " is merged but not in the vocab: its id is unk's, its span stays
        vocab.setdefault(l + r, 256 + len(vocab))
    tok = BBPETokenizer(vocab={**vocab, b"<s>": 900}, merges=merges, special_tokens=["<s>", "<t>"])
    rng = random.Random(4)
    words = ["".join(rng.choice("ab") for _ in range(n)) for n in (63, 64, 65, 66, 130)]  # 64: the last lane word; 65: the first long one
    check(tok, words + ["é" * 32, "é" * 33, " " * 64, " " * 65, " ".join(words)], "path boundary")
    ids, _off, spans = BBPETokenizer(vocab=dict(IDENT), merges=[]).encode_array_with_offsets(["a\U0001F600"], "char")
    assert ids.tolist() == [0x61, 0xF0, 0x9F, 0x98, 0x80] and spans.tolist() == [[0, 1]] + [[1, 2]] * 4  # one character over four tokens
    check(tok, ["", "ab<s>é<t>ab", "", "é中\U0001F600a 1'", ""], "empty first and last document")
    check(tok, ["", ""], "only empty documents")
    check(tok, [rng.choice(["é", "ab ", "<s>", "<t>x", "中 b", "", "\U0001F600"]) * rng.randint(0, 3) for _ in range(3000)], "3000 documents")
    big = "".join(rng.choice(["é", "中", "\U0001F600", "中中 ", "ab", "éé", " "]) for _ in range(60_000))
    assert 180_000 < len(big.encode("utf-8")) < 220_000
    check(tok, ["x", big, "é"], "200 KB of multi-byte text")


def test_scale_without_python_per_token():
    from yet_another_bpe import _native

    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, 4 << 20)
        vocab, merges, ctx = encode_helpers.train_on_device(gen, tb, tn, 2000)
        ctx.close()
        data = gen.d2h(tb, tn).tobytes()
    cut = [0]  # 64 documents, cut at character starts
    for k in range(1, 64):
        p = k * tn // 64
        while data[p] & 0xC0 == 0x80:
            p += 1
        cut.append(p)
    blobs = [data[a:b] for a, b in zip(cut, cut[1:] + [tn])]
    docs = [b.decode("utf-8") for b in blobs]
    tok = BBPETokenizer(vocab=vocab, merges=merges)
    ids, off, spans = tok.encode_array_with_offsets(docs, "byte")
    pids, poff = tok.encode_array(docs)
    assert np.array_equal(ids, pids) and np.array_equal(off, poff) and spans.shape == (len(ids), 2)
    o = off.astype(np.int64)
    assert np.all(np.diff(o) > 0)
    assert np.all(spans[o[:-1], 0] == 0)  # every document: starts at 0 ...
    assert np.array_equal(spans[o[1:] - 1, 1], np.asarray([len(b) for b in blobs], dtype=np.uint64))  # ... ends at its length ...
    inner = np.ones(len(ids), dtype=bool)
    inner[o[1:] - 1] = False
    assert np.array_equal(spans[inner, 1], spans[np.flatnonzero(inner) + 1, 0])  # ... and tiles in between
    tlen = np.zeros(max(vocab.values()) + 1, dtype=np.uint64)
    for t, i in vocab.items():
        tlen[i] = len(t)
    assert np.array_equal(spans[:, 1] - spans[:, 0], tlen[ids])  # every token is in the vocab: its span is its length
    head = 0
    while sum(len(b) for b in blobs[:head]) < 256 << 10:
        head += 1
    for unit in UNITS:
        gids, goff, gspans = tok.encode_array_with_offsets(docs, unit) if unit == "char" else (ids, off, spans)
        eids, eoff, espans = flat(tok.encode_batch_with_offsets(docs[:head], unit))
        k = int(eoff[-1])
        assert np.array_equal(gids[:k], eids) and np.array_equal(goff[:head + 1], eoff) and np.array_equal(gspans[:k], espans), unit


def test_errors_and_no_side_effects():
    import ctypes

    from yet_another_bpe import _native

    tok = BBPETokenizer(vocab=dict(IDENT), merges=[(b"a", b"b")], special_tokens=["<s>"])
    before = tok.encode_array(["ab<s>ab é", "", "x"])
    for b in [b"\x80", b"ab\xc3", b"\xe2\x82<s>", b"<s>\x80", b"ok<s>\xc3\xa9\xa9"]:
        with pytest.raises(UnicodeDecodeError) as e:
            b.decode("utf-8")
        for unit in UNITS:
            with pytest.raises(_native.Utf8Error) as g:
                tok.encode_array_with_offsets(b, unit)
            assert g.value.position == e.value.start, (b, unit)
    for unit in UNITS:
        ids, off, spans = tok.encode_array_with_offsets([], unit)
        assert ids.shape == (0,) and off.tolist() == [0] and spans.shape == (0, 2) and spans.dtype == np.uint64
        assert tok.encode_batch_device_with_offsets([], unit) == []
        assert tok.encode_batch_device_with_offsets(["", "", "ab", "<s>"], unit) == [([], []), ([], []), ([0], [(0, 2)]), ([], [])]
    with pytest.raises(ValueError):
        tok.encode_array_with_offsets(["ab"], unit="x")
    after = tok.encode_array(["ab<s>ab é", "", "x"])  # a plain call after the spans calls
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    with _native.Context() as ctx:  # no model
        with pytest.raises(_native.YabpeError) as e:
            ctx.encode_spans(b"ab")
        assert e.value.code == -1
        di, dd, ds, ni, bad = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_int64(-1)
        docs = np.zeros(1, dtype=np.uint64)
        ctx.encode_set_model(dict(IDENT), [], [], 0)
        rc = _native.lib().yabpe_encode_spans(ctx._h, b"ab", 2, docs.ctypes.data, 1, 0x2, ctypes.byref(di), ctypes.byref(dd), ctypes.byref(ds),
                                              ctypes.byref(ni), ctypes.byref(bad))
        assert rc == -1 and not ds.value  # an unknown flag


def test_device_text_at_an_unaligned_address():
    """The char unit reads the text in aligned 16-byte chunks; resident text that starts elsewhere gives the same spans."""
    from yet_another_bpe import _native

    tok = BBPETokenizer(vocab={**IDENT, b"th": 256, b"\xc3\xa9": 257}, merges=[(b"t", b"h"), (b"\xc3", b"\xa9")])
    with _native.Context() as gen:
        tb, tn = encode_helpers.lexicon_text(gen, 64 << 10)
        data = gen.d2h(tb, tn).tobytes()
        k = next(k for k in range(1, 16) if data[k] & 0xC0 != 0x80)
        gen.encode_set_model(tok._vocab, tok._merges, [], 0)
        for unit in UNITS:
            ids, off, spans = gen.encode_spans_to_host(tb + k, n_bytes=tn - k, chars=unit == "char")
            eids, espans = tok.encode_with_offsets(data[k:].decode("utf-8"), unit)
            assert ids.tolist() == eids and off.tolist() == [0, len(eids)] and [tuple(p) for p in spans.tolist()] == espans, unit
